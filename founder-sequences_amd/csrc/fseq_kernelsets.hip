// fseq_kernelsets.hip -- the kernel configurations of the path and their launchers: the LDS-resident column / chain / rank
// kernels by row count (select_kernels); phase A's key-space tree and trie by workgroup size and the streamed phase C's tile
// configuration (stream2_config) are csrc/fseq_kernelsets_stream.hip.  A translation unit of its own since round 5 (the review's "split fseq_api.hip"): these
// template instantiations were two thirds of what a rebuild of csrc/fseq_api.hip cost, and nothing in the orchestration
// touches them but through the function tables of fseq_ctx.hpp (KernelSet, Stream2Config).  A launcher takes the views of
// fseq_types.hpp (the alignment, the key blocks, the lists, ...) and is the one place that writes out its kernel's parameter list.
#include "fseq_ctx.hpp"
#include "fseq_kernels.hpp"

#include <cstdio>

namespace fseq {

namespace {

// EW: phase C keeps wave 0 free of rows for the per-column list (k_columns, fseq_kernels.hpp): m <= (T - 64) * E
template <int T, int E, int SIGMA, bool PK, bool EW = false>
struct Launch {
	static void rank(hipStream_t st, uint32_t grid, size_t lds, PhaseAArgs const &K)
	{
		MsaArgs const &A = K.A;
		// (only: the per-block filter goes in the start-state slot, which the rank mode does not use otherwise -- k_colblock)
		hipLaunchKernelGGL((k_colblock<T, E, SIGMA, MODE_RANK, PK>), dim3(grid), dim3(T), lds, st, A.msa, A.ld, A.m, A.n, A.B, A.nblocks, A.npass, A.bsh, K.rank, K.keyd, K.nkeys,
		                   K.only, (uint32_t const *) nullptr, (uint64_t const *) nullptr, (uint2 const *) nullptr,
		                   (uint32_t *) nullptr, (uint32_t *) nullptr, (uint64_t const *) nullptr, 0u, (uint32_t const *) nullptr, (uint32_t const *) nullptr, K.col0,
		                   (uint64_t) A.B < (1ull << scan_shift_for(T, E)) ? 1u : 0u);      // (divergences relative to the block start: <= B)
	}
	static void snap(hipStream_t st, uint32_t grid, size_t lds, SnapArgs const &S)
	{
		MsaArgs const &A = S.A;
		hipLaunchKernelGGL((k_colblock<T, E, SIGMA, MODE_SNAP, PK>), dim3(grid), dim3(T), lds, st, A.msa, A.ld, A.m, A.n, A.B, A.nblocks, A.npass, A.bsh,
		                   (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, S.bstate_a, S.bstate_d, S.task_rb, S.task_grp, S.snap_a, S.snap_d,
		                   S.task_src, S.ss.snap_stride, (uint32_t const *) S.ss.ss_a, (uint32_t const *) S.ss.ss_d, (uint64_t) 0, S.keyed);
	}
	static size_t columns_lds(uint32_t B) { return columns_lds_bytes<T, E, SIGMA, PK>(B); }
	template <bool DENSE>
	static void columns_as(hipStream_t st, uint32_t grid, size_t lds, ColumnsArgs const &C)
	{
		MsaArgs const &A = C.A;
		hipLaunchKernelGGL((k_columns<T, E, SIGMA, PK, EW, DENSE>), dim3(grid), dim3(T), lds, st, A.msa, A.ld, A.m, A.n, A.B, A.N2, C.bstate_a, C.bstate_d,
		                   C.lists.L, C.lists.X, C.lists.stride, C.lists.ent, C.lists.hdr, A.npass, A.bsh, C.ss.snap_stride, C.ss.ss_a, C.ss.ss_d,
		                   C.block0, C.done_host, C.epoch, C.colmask, C.blocklist);
	}
	static void columns(hipStream_t st, uint32_t grid, size_t lds, ColumnsArgs const &C)
	{
		if (C.colmask) columns_as<true>(st, grid, lds, C);
		else columns_as<false>(st, grid, lds, C);
	}
	static uint32_t columns_resident(size_t lds)
	{
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_columns<T, E, SIGMA, PK, EW>, T, lds) != hipSuccess || nb < 1) nb = 1;
		return (uint32_t) nb;
	}
	static void chain(hipStream_t st, uint32_t grid, size_t lds, ChainMultiArgs const &C, uint32_t keyed)
	{
		hipLaunchKernelGGL((k_chain<T, E, PK>), dim3(grid), dim3(T), lds, st, C.rank, C.keyd, C.nkeys, C.m, C.nb_total, C.G, C.cols_per_block,
		                   C.start_a, C.start_d, C.out_state_a, C.out_state_d, C.out_rank, C.out_keyd, C.out_nkeys, C.grp0, keyed);
	}
	static hipError_t prepare()
	{
		hipError_t e;
		if ((e = allow_lds(k_colblock<T, E, SIGMA, MODE_RANK, PK>, colblock_lds_bytes<T, E, SIGMA, MODE_RANK, PK>())) != hipSuccess) return e;
		if ((e = allow_lds(k_colblock<T, E, SIGMA, MODE_SNAP, PK>, colblock_lds_bytes<T, E, SIGMA, MODE_SNAP, PK>())) != hipSuccess) return e;
		return allow_lds(k_chain<T, E, PK>, chain_lds_bytes<T, E, PK>());
	}
	static hipError_t prepare_columns(size_t lds_columns)
	{
		hipError_t const e = allow_lds(k_columns<T, E, SIGMA, PK, EW, false>, lds_columns);
		return e != hipSuccess ? e : allow_lds(k_columns<T, E, SIGMA, PK, EW, true>, lds_columns);
	}
	static KernelSet make()
	{
		KernelSet k;
		k.T = T; k.E = E; k.sigma = SIGMA; k.cap = T * E; k.scan_shift = (uint32_t) scan_shift_for(T, E);
		k.lds_colblock = colblock_lds_bytes<T, E, SIGMA, MODE_RANK, PK>();
		k.lds_snap = colblock_lds_bytes<T, E, SIGMA, MODE_SNAP, PK>();
		k.rank = &rank; k.snap = &snap; k.columns_lds = &columns_lds; k.columns = &columns; k.columns_resident = &columns_resident;
		k.lds_chain = chain_lds_bytes<T, E, PK>();
		k.chain = &chain; k.prepare = &prepare; k.prepare_columns = &prepare_columns;
		return k;
	}
};

// phase C from another configuration than phases A, B and pass 2 (the emitter-wave kernels give their threads one
// row more; the latency-bound chain and snapshot kernels are better off without it)
template <typename Base, typename Col>
KernelSet compose_kernels()
{
	KernelSet k = Base::make();
	k.columns_lds = &Col::columns_lds; k.columns = &Col::columns; k.columns_resident = &Col::columns_resident; k.prepare_columns = &Col::prepare_columns;
	return k;
}

} // namespace

bool select_kernels(uint32_t m, uint32_t sigma, KernelSet *out)
{
	if (sigma > 256) return false;
	// 1024-thread configurations spare wave 0 for the per-column lists when the rows allow it (measured: C5 phase C
	// 86 -> 75 ms with it, while 512-thread workgroups lose as much to the longer per-thread chunks as they gain)
#define FSEQ_TRY_EW(T_, E_, PK_)                                                               \
	if (m <= (uint32_t) ((T_) - 64) * (E_))                                                    \
	{                                                                                          \
		*out = Launch<T_, E_, 4, PK_, true>::make();                                            \
		return true;                                                                           \
	}
#define FSEQ_TRY(T_, E_, PK_)                                                                  \
	if (m <= (uint32_t) (T_) * (E_))                                                           \
	{                                                                                          \
		*out = Launch<T_, E_, 4, PK_>::make();                                                  \
		return true;                                                                           \
	}
	FSEQ_TRY(64, 1, false)
	FSEQ_TRY(64, 7, false)
	FSEQ_TRY(256, 5, false)
	// 512 threads: the list wave pays since the partition step's scan became cheap (BASELINE C3: phase C 8.2 -> 7.7 ms
	// with six rows on seven waves and the list on the eighth; 576 threads would keep five rows per thread, but nine
	// waves per workgroup place three on one SIMD and only one workgroup fits a CU)
	// [late r3] ... with 16-bit LDS words (value ids are < m + B < 65536 anyway): 48 KiB instead of 70 per workgroup and 80
	// registers by launch bounds put THREE workgroups on a CU -- a column step is a chain of three barriers and ~6 LDS round
	// trips, and two workgroups left the SIMDs idle 43 % of the time (BASELINE C3: phase C 5.61 -> 5.08 ms; the unpacking
	// costs less than the third workgroup brings)
	if (m > 448u * 5u && m <= 448u * 6u && m <= 512u * 5u)
	{
		*out = compose_kernels<Launch<512, 5, 4, false>, Launch<512, 6, 4, true, true>>();
		return true;
	}
	if (m > 256u * 5u && m <= 448u * 5u)
	{
		*out = compose_kernels<Launch<512, 5, 4, false>, Launch<512, 5, 4, true, true>>();
		return true;
	}
	FSEQ_TRY(512, 5, false)
	FSEQ_TRY(512, 7, false)
	FSEQ_TRY_EW(1024, 5, false)    // (3,585 .. 5,120 rows: e.g. the 5,008 haplotypes of 2,504 diploid samples)
	FSEQ_TRY(1024, 5, false)
	FSEQ_TRY_EW(1024, 7, false)
	FSEQ_TRY(1024, 7, false)
	// 16-bit LDS state (m <= 11,264).  These kernels want more registers than a wave of a 1024-thread workgroup gets
	// (~13 per row of E): the fewest rows per thread that hold m, the list wave where the same E allows it
	// (BASELINE C5, m = 10,000: (1024,10) 56.9 ms of phase C against 61.9 with (1024,11) and the list wave)
	FSEQ_TRY_EW(1024, 9, true)
	FSEQ_TRY(1024, 9, true)
	FSEQ_TRY_EW(1024, 10, true)
	FSEQ_TRY(1024, 10, true)
	FSEQ_TRY_EW(1024, 11, true)
	FSEQ_TRY(1024, 11, true)
#undef FSEQ_TRY
#undef FSEQ_TRY_EW
	return false;
}


} // namespace fseq
