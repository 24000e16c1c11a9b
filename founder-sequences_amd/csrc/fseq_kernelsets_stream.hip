// fseq_kernelsets_stream.hip -- launchers by configuration, second part (csrc/fseq_kernelsets.hip): phase A's key-space tree
// (k_blockkeys) and trie (k_blocktrie) by workgroup size and bits per symbol, the streamed phase C's tile configurations
// (k_columns_stream2, stream2_config).  They take the views of fseq_types.hpp, as the launchers of the first part do.
#include "fseq_ctx.hpp"
#include "fseq_kernels.hpp"
#include "fseq_stream.hpp"
#include "fseq_stream2.hpp"
#include "fseq_blockkeys.hpp"
#include "fseq_blocktrie.hpp"

#include <cstdio>

namespace fseq {

namespace {

// phase C, streamed rows, second form (fseq_stream2.hpp): T threads x E rows of 5 bytes (the one configuration; the 8-byte
// rows and the other tile shapes are gone: no default decision picked them)
constexpr int S2_T = 512, S2_E = 8;
size_t s2_lds(uint32_t colbytes) { return stream2_lds_bytes<S2_T, S2_E>(colbytes); }
hipError_t s2_prepare(size_t bytes)
{
	hipError_t const e = allow_lds(k_columns_stream2<S2_T, S2_E>, bytes);
	if (e != hipSuccess) return e;
	return allow_lds(k_columns_stream2<S2_T, S2_E, S2_SNAP>, bytes);
}
void s2_launch_snap(hipStream_t st, uint32_t grid, size_t bytes, SnapArgs const &S)
{
	MsaArgs const &A = S.A;
	S2SnapArgs SN{};
	SN.wg_block = S.wg_block; SN.wg_groups = S.wg_groups; SN.grp_tasks = S.task_grp; SN.grp_src = S.task_src; SN.task_rb = S.task_rb;
	SN.snap_a = S.snap_a; SN.snap_d = S.snap_d; SN.bs_w = S.bs_w; SN.bs_h = S.bs_h;
	// (no lists, no launch window)
	hipLaunchKernelGGL((k_columns_stream2<S2_T, S2_E, S2_SNAP>), dim3(grid), dim3(S2_T), bytes, st, A.msa, A.ld, A.m, A.n, A.B, A.npass, A.bsh, S.ws, 0u, 0u, 0u, (uint2 *) nullptr, (uint4 *) nullptr,
	                   S.ss.snap_stride, S.ss.ss_a, S.ss.ss_d, 0u, (uint32_t *) nullptr, 0u, 0u, SN);
}
void s2_launch(hipStream_t st, uint32_t grid, size_t bytes, ColumnsArgs const &C)
{
	MsaArgs const &A = C.A;
	S2SnapArgs SN{};
	SN.wg_block = C.blocklist;
	hipLaunchKernelGGL((k_columns_stream2<S2_T, S2_E>), dim3(grid), dim3(S2_T), bytes, st, A.msa, A.ld, A.m, A.n, A.B, A.npass, A.bsh, C.ws, C.lists.L, C.lists.X, C.lists.stride, C.lists.ent, C.lists.hdr,
	                   C.ss.snap_stride, C.ss.ss_a, C.ss.ss_d, C.block0, C.done_host, C.epoch, C.ss.ss_pack | (C.ss.ids ? S2_SS_IDS : 0u), SN);
}
uint32_t s2_resident(size_t bytes)
{
	int nb = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_columns_stream2<S2_T, S2_E>, S2_T, bytes) != hipSuccess || nb < 1) nb = 1;
	return (uint32_t) nb;
}
} // namespace

// phase A in key space, LDS-resident rows (fseq_blockkeys.hpp): the kernel has its own workgroup size, one thread
// per 8 rows where that fits (blockkeys_threads)
#define FSEQ_BK_SIZES(X) X(256) X(320) X(512) X(768) X(1024)
void launch_blockkeys(hipStream_t st, uint32_t grid, size_t lds, PhaseAArgs const &K)
{
	MsaArgs const &A = K.A;
	switch (K.T)
	{
#define X(T_) case T_: hipLaunchKernelGGL((k_blockkeys<T_>), dim3(grid), dim3(T_), lds, st, A.msa, A.ld, A.m, A.n, A.B, A.bsh, K.rank, K.keyd, K.nkeys, K.col0, \
	                                          static_cast<uint16_t *>(K.work), K.work_per, K.cap_words, K.counters, K.todo, K.only); break;
		FSEQ_BK_SIZES(X)
#undef X
		default: break;
	}
}
hipError_t prepare_blockkeys(uint32_t T, size_t lds, bool debug)
{
	if (debug)
	{
		int nb = -1;
		switch (T)
		{
#define X(T_) case T_: (void) allow_lds(k_blockkeys<T_>, lds); (void) hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_blockkeys<T_>, T_, lds); break;
			FSEQ_BK_SIZES(X)
#undef X
			default: break;
		}
		fprintf(stderr, "fseq: k_blockkeys<%u> with %zu bytes of LDS: %d workgroups per CU\n", T, lds, nb);
	}
	switch (T)
	{
#define X(T_) case T_: return allow_lds(k_blockkeys<T_>, lds);
		FSEQ_BK_SIZES(X)
#undef X
		default: return hipErrorInvalidValue;
	}
}

// phase A, the trie over 32-bit group words (fseq_blocktrie.hpp): T threads by the row count (12 T classes fit), bits per symbol
uint32_t blocktrie_threads(uint32_t m, bool stream) { return stream || m > 12u * 512u ? 1024u : m > 12u * 256u ? 512u : 256u; }
size_t blocktrie_lds(uint32_t T) { return T == 256u ? BtGeom<256>::LDS_BYTES : T == 512u ? BtGeom<512>::LDS_BYTES : BtGeom<1024>::LDS_BYTES; }
hipError_t launch_blocktrie(hipStream_t st, uint32_t groups, PhaseAArgs const &K)
{
	MsaArgs const &A = K.A;
	uint32_t const bits = 8u >> A.bsh;
#define FSEQ_BT_LAUNCH(BITS_, T_, CLS_) \
	{ \
		hipError_t const e = allow_lds(k_blocktrie<BITS_, T_, CLS_>, BtGeom<T_>::LDS_BYTES); \
		if (e != hipSuccess) return e; \
		hipLaunchKernelGGL((k_blocktrie<BITS_, T_, CLS_>), dim3(groups), dim3(T_), BtGeom<T_>::LDS_BYTES, st, A.msa, A.ld, A.m, A.n, A.B, K.nblk, K.rank, K.keyd, K.nkeys, K.col0, \
		                   static_cast<uint32_t *>(K.work), K.work_per, K.counters, K.todo, K.cls, K.ldc, K.cls_have); \
		return hipSuccess; \
	}
	// (the kernel with the class columns' phase is an instantiation of its own: where nobody reads them -- K.cls == nullptr -- the kernel is
	// instruction for instruction the one without that phase.  Class columns are written for streamed rows only, and those run 1,024 threads)
#define FSEQ_BT_CASE(BITS_, T_) \
	if (bits == BITS_ && K.T == T_) \
	{ \
		if constexpr (T_ == 1024) { if (K.cls) FSEQ_BT_LAUNCH(BITS_, T_, true) } \
		else if (K.cls) return hipErrorInvalidValue; \
		FSEQ_BT_LAUNCH(BITS_, T_, false) \
	}
	FSEQ_BT_CASE(2, 256) FSEQ_BT_CASE(2, 512) FSEQ_BT_CASE(2, 1024)
	FSEQ_BT_CASE(4, 256) FSEQ_BT_CASE(4, 512) FSEQ_BT_CASE(4, 1024)
	FSEQ_BT_CASE(8, 256) FSEQ_BT_CASE(8, 512) FSEQ_BT_CASE(8, 1024)
#undef FSEQ_BT_CASE
#undef FSEQ_BT_LAUNCH
	return hipErrorInvalidValue;
}

Stream2Config stream2_config()
{
	return Stream2Config{(uint32_t) S2_T, (uint32_t) S2_E, (uint32_t) s2_key_shift(S2_T * S2_E), &s2_lds, &s2_prepare, &s2_launch, &s2_resident, &s2_launch_snap};
}



} // namespace fseq
