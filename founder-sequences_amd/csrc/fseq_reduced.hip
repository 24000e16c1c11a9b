// fseq_reduced.hip -- [r5] the kernels of phase C / pass 2 on representative rows (fseq_reduced.hpp) and their launchers: a
// translation unit of its own, compiled beside the units of the path (which reach them through the function tables below).
#include "fseq_ctx.hpp"
#include "fseq_reduced.hpp"

namespace fseq {

namespace {

template <int T, int E, bool PK, bool EW>
struct LaunchRed {
	static size_t lds(uint32_t B, uint32_t symcap)
	{
		return columns_lds_bytes<T, E, 4, PK>(B) - 2 * carve_bytes((size_t) T * E, 1) + 2 * carve_bytes(symcap, 1);
	}
	// [r16] the forms compiled: phase C's where the plan sends phase C (plan_reduced: T <= 128 || ew), the sweep form where it sends
	// pass 2 (!ew) -- only the 64-thread configurations have both
	static constexpr bool PHASE = T <= 128 || EW, SWEEP = !EW;
	static size_t lds_sweep(uint32_t, uint32_t symcap)
	{
		size_t const runs = columns_run_words(T, E, 4, PK);
		return 2 * carve_bytes((size_t) T * E, PK ? 2 : 4) + 2 * carve_bytes(symcap, 1) + carve_bytes(1, sizeof(StepScratch<T, 4>)) + carve_bytes(T / WAVE + 1, 4)
		     + (runs ? carve_bytes(runs, 4) : 0);
	}
	static hipError_t prepare(size_t bytes, bool sweep)
	{
		if constexpr (SWEEP) { if (sweep) return allow_lds(k_columns_red<T, E, 4, PK, EW, true>, bytes); }
		if constexpr (PHASE) { if (!sweep) return allow_lds(k_columns_red<T, E, 4, PK, EW>, bytes); }
		return hipErrorInvalidDeviceFunction;               // (a form this configuration is never planned for)
	}
	static hipError_t launch(hipStream_t st, uint32_t grid, size_t bytes, ColumnsArgs const &C, RedArgs const &red)
	{
		MsaArgs const &A = C.A;
		bool launched = false;
		if constexpr (SWEEP)
		{
			if (red.cls)
			{
				launched = true;
				hipLaunchKernelGGL((k_columns_red<T, E, 4, PK, EW, true>), dim3(grid), dim3(T), bytes, st, A.msa, A.ld, A.n, A.B, C.lists.L, C.lists.X, C.lists.stride, C.lists.ent,
				                   C.lists.hdr, A.npass, A.bsh, red);
			}
		}
		if constexpr (PHASE)
		{
			if (!red.cls)
			{
				launched = true;
				hipLaunchKernelGGL((k_columns_red<T, E, 4, PK, EW>), dim3(grid), dim3(T), bytes, st, A.msa, A.ld, A.n, A.B, C.lists.L, C.lists.X, C.lists.stride, C.lists.ent, C.lists.hdr,
				                   A.npass, A.bsh, red);
			}
		}
		return launched ? hipSuccess : hipErrorInvalidDeviceFunction;      // (a form this configuration does not have: nothing was launched)
	}
	// (a configuration that has the sweep form only answers for that kernel at the bytes asked for.  Planning asks with phase C's LDS
	// figure -- red_configs' class-column rule and red_report's line --, which is more than a sweep requests: the answer is a lower
	// bound of the sweeps' residents, kept so that which blocks stage their class columns does not move with [r16])
	static uint32_t resident(size_t bytes)
	{
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_columns_red<T, E, 4, PK, EW, !PHASE>, T, bytes) != hipSuccess || nb < 1) nb = 1;
		return (uint32_t) nb;
	}
	static ReducedSet make()
	{
		return ReducedSet{(uint32_t) T, (uint32_t) E, EW ? (uint32_t) (T - 64) * E : (uint32_t) T * E, (uint32_t) columns_value_cap(T, E, PK), PK, EW, &lds, &lds_sweep, &prepare, &launch, &resident};
	}
};

// ascending by the rows they hold.  EW: wave 0 holds no rows and emits the lists while the row waves are in the next column (from 256
// threads on: what phase C runs -- the lists of a block with thousands of representatives are a thousand entries long, and
// on a wave that also holds rows they were 40 % of a column of BASELINE C4 --; pass 2's sweeps, which emit none, take the others).
// Small blocks run one wave for both.
// [r7] 512 x 15 (the slim configuration, fseq_kernels.hpp: two workgroups per CU) stands in front of 1024 x 7, which holds the same
// rows: the plan takes the first configuration that holds a block, and 1024 x 7 the blocks the slim one refuses.
#define FSEQ_RED_CONFIGS(X) \
	X(64, 3, false, false) X(64, 5, false, false) X(64, 7, false, false) \
	X(256, 3, false, true) X(256, 3, false, false) X(256, 5, false, true) X(256, 5, false, false) X(512, 5, false, true) X(512, 5, false, false) \
	X(512, 7, false, true) X(512, 7, false, false) X(1024, 5, false, true) X(1024, 5, false, false) X(512, 15, true, true) X(1024, 7, true, true) X(1024, 7, true, false) \
	X(1024, 8, true, true) X(1024, 9, true, true) X(1024, 9, true, false) X(1024, 10, true, true) X(1024, 10, true, false) X(1024, 11, true, true) \
	X(1024, 11, true, false) X(1024, 12, true, true)

template <int T, int E, bool PK>
struct LaunchChainSnap {
	static hipError_t prepare() { return allow_lds(k_chain_snap<T, E, PK>, chain_snap_lds_bytes<T, E, PK>()); }
	static void launch(hipStream_t st, uint32_t grid, size_t bytes, SnapArgs const &S, RedArgs const &red)
	{
		hipLaunchKernelGGL((k_chain_snap<T, E, PK>), dim3(grid), dim3(T), bytes, st, S.bstate_a, S.bstate_d, red.rank, red.m_true, S.task_blk, (uint32_t const *) red.cls,
		                   (uint32_t const *) red.headd, (uint32_t const *) red.ncls, red.cap, S.snap_a, S.snap_d, S.keyed);
	}
	static ChainSnapSet make() { return ChainSnapSet{chain_snap_lds_bytes<T, E, PK>(), &prepare, &launch}; }
};

// the base configurations of select_kernels (fseq_kernelsets.hip)
#define FSEQ_CHAIN_SNAP_CONFIGS(X) \
	X(64, 1, false) X(64, 7, false) X(256, 5, false) X(512, 5, false) X(512, 7, false) X(1024, 5, false) X(1024, 7, false) X(1024, 9, true) X(1024, 10, true) X(1024, 11, true)

} // namespace

int reduced_config_count()
{
	int n = 0;
#define X(T_, E_, PK_, EW_) ++n;
	FSEQ_RED_CONFIGS(X)
#undef X
	return n;
}

bool reduced_config(int index, ReducedSet *out)
{
	int i = 0;
#define X(T_, E_, PK_, EW_) if (i++ == index) { *out = LaunchRed<T_, E_, PK_, EW_>::make(); return true; }
	FSEQ_RED_CONFIGS(X)
#undef X
	return false;
}

bool select_chain_snap(uint32_t T, uint32_t E, ChainSnapSet *out)
{
#define X(T_, E_, PK_) if (T == T_ && E == E_) { *out = LaunchChainSnap<T_, E_, PK_>::make(); return true; }
	FSEQ_CHAIN_SNAP_CONFIGS(X)
#undef X
	return false;
}

hipError_t launch_reduce_prep(hipStream_t st, uint32_t grid, RedPrepArgs const &A)
{
	size_t const bytes = reduce_prep_lds_bytes(A.m);
	if (bytes > 160 * 1024) return hipErrorInvalidValue;
	hipError_t const e = allow_lds(k_reduce_prep, bytes);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_reduce_prep, dim3(grid), dim3(RED_PREP_T), bytes, st, A);
	return hipSuccess;
}

void launch_reduce_check(hipStream_t st, uint32_t const *cnt, uint32_t const *planned, uint32_t count, uint32_t *flags)
{
	if (count) hipLaunchKernelGGL(k_reduce_check, dim3((count + 255u) / 256u), dim3(256), 0, st, cnt, planned, count, flags);
}

template <int BSH, int R>
static bool launch_reduce_msa_lds(hipStream_t st, MsaArgs const &A, ReducedMsaArgs const &D, uint32_t colbytes)
{
	static bool prepared = false;
	size_t const lds = (size_t) 2 * R * 16384;
	if (!prepared)
	{
		if (hipFuncSetAttribute(reinterpret_cast<void const *>(&k_reduce_msa_lds<BSH, R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
		{
			(void) hipGetLastError();
			return false;
		}
		prepared = true;
	}
	// (a quarter of a block's columns per workgroup: the rows are read four times, the blocks' columns are enough workgroups)
	hipLaunchKernelGGL((k_reduce_msa_lds<BSH, R>), dim3(D.nlisted, 4), dim3(1024), lds, st, A.msa, A.ld, D.red, D.ldr, D.cnt, D.rows, D.cap, A.n, A.B, D.blocks, colbytes, D.flag, D.want, D.pad, D.pad_per, D.skip);
	return true;
}

void launch_reduce_msa(hipStream_t st, MsaArgs const &A, ReducedMsaArgs const &D, bool gather_only)
{
	if (!D.nlisted) return;
	uint32_t const colbytes = sym_bytes(A.m, A.bsh);
	// the column through LDS where it fits two buffers of at most 32 KB and the representatives the registers of 1,024 threads
	if (!gather_only && colbytes <= 32768u && D.cap <= 12288u)
	{
		bool const one = colbytes <= 16384u;
		bool ok = false;
		switch (A.bsh)
		{
		case 0: ok = one ? launch_reduce_msa_lds<0, 1>(st, A, D, colbytes) : launch_reduce_msa_lds<0, 2>(st, A, D, colbytes); break;
		case 1: ok = one ? launch_reduce_msa_lds<1, 1>(st, A, D, colbytes) : launch_reduce_msa_lds<1, 2>(st, A, D, colbytes); break;
		case 2: ok = one ? launch_reduce_msa_lds<2, 1>(st, A, D, colbytes) : launch_reduce_msa_lds<2, 2>(st, A, D, colbytes); break;
		default: break;
		}
		if (ok) return;
	}
	uint32_t const nq = (D.max_rows + (1u << A.bsh) - 1u) >> A.bsh;
	hipLaunchKernelGGL(k_reduce_msa, dim3(D.nlisted, (nq + 63u) / 64u), dim3(256), 0, st, A.msa, A.ld, D.red, D.ldr, D.cnt, D.rows, D.cap, A.n, A.B, A.bsh, D.blocks, D.flag, D.want);
}

// the listed blocks that have class columns, from those: k_reduce_msa_lds with the class columns as its alignment and the representatives' leaf
// ranks as its rows (false: a shape that kernel does not take -- nothing is launched, the caller reads the alignment)
bool launch_reduce_cls(hipStream_t st, MsaArgs const &A, ReducedMsaArgs const &D, ClassColumnArgs const &K)
{
	if (!D.nlisted) return true;
	if (K.ldc > 16384u || D.cap > 12288u || A.bsh > 2u) return false;
	MsaArgs S = A;
	S.msa = K.cls; S.ld = K.ldc;
	ReducedMsaArgs E = D;
	E.rows = K.leaf; E.flag = K.have; E.want = 1u; E.pad = K.rank; E.pad_per = A.m;
	switch (A.bsh)
	{
	case 0: return launch_reduce_msa_lds<0, 1>(st, S, E, (uint32_t) K.ldc);
	case 1: return launch_reduce_msa_lds<1, 1>(st, S, E, (uint32_t) K.ldc);
	default: return launch_reduce_msa_lds<2, 1>(st, S, E, (uint32_t) K.ldc);
	}
}

} // namespace fseq
