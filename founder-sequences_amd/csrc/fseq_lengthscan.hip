// fseq_lengthscan.hip -- the segment length as a parameter of a resident alignment: fseq_set_segment_length (another L on the
// context), fseq_scan_segment_lengths (the maximum segment size at several lengths: phases A and B once, the lists built at the
// smallest length and folded from each length to the next, the DP alone per length), and their debug entry points.  The one unit
// that includes fseq_lengthscan.hpp (k_relump_lists); the attempt's stages it shares with a run are csrc/fseq_path_attempt.hip's
// (long_attempts_to_proof, long_dp_on_lists), the order of work is a pure host function (plan_length_scan, fseq_scanplan.hpp).
#include "fseq_path.hpp"
#include "fseq_lengthscan.hpp"
#include "fseq_scanplan.hpp"

namespace fseq {

void launch_relump_lists(hipStream_t st, RelumpArgs const &R)
{
	if (!R.ncols) return;
	uint32_t const grid = (uint32_t) ((R.ncols + RELUMP_WAVES - 1) / RELUMP_WAVES);
	hipLaunchKernelGGL(k_relump_lists, dim3(grid), dim3(64 * RELUMP_WAVES), 0, st, R.lists.ent, R.lists.hdr, R.lists.stride, R.lists.L, R.k0, R.ncols);
}

// The DP arrays are sized by n - L + 1 where the geometry's buffers are allocated (alloc_geometry_buffers); a context that holds
// those already grows them here and never shrinks them.  A failed allocation drops the work buffers: the next run allocates afresh.
int apply_segment_length(fseq_ctx *c, uint64_t L)
{
	c->p.segment_length = L;
	if (scan_short_path(c->p.n, L)) return FSEQ_OK;               // (n < 2L: one sweep, no DP)
	c->dp_size = c->p.n - L + 1;
	c->dp.tstride = (uint32_t) (c->dp_size / 64 + 2);
	if (!c->d_rank) return FSEQ_OK;
	int rc;
	if ((rc = c->dp.M.ensure(c, c->dp_size)) || (rc = c->dp.LB.ensure(c, c->dp_size)) || (rc = c->dp.SZ.ensure(c, c->dp_size))
	    || (rc = c->dp.K.ensure(c, c->dp_size + 64)) || (rc = c->dp.Tb.ensure(c, (size_t) 32 * c->dp.tstride))
	    || (rc = c->dp.Tbv.ensure(c, (size_t) 32 * c->dp.tstride)) || (rc = c->d_Mprev.ensure(c, c->dp_size)))
	{
		std::string const keep = c->err;
		free_work(c);
		c->err = keep;
		return rc;
	}
	return FSEQ_OK;
}

namespace {

struct ScanSlot {                            // what the scan found at one distinct long-path length
	uint32_t max_segment_size = 0, lists = FSEQ_SCAN_LISTS_BUILT, list_cap = 0, dp_chunks = 0;
	double ms = 0;
};

struct ScanEvents {
	hipEvent_t begin = nullptr, end = nullptr;
	~ScanEvents() { if (begin) (void) hipEventDestroy(begin); if (end) (void) hipEventDestroy(end); }
};

// the time between the two events, once the second has happened
int scan_elapsed(fseq_ctx *c, ScanEvents const &ev, double *ms)
{
	float f = 0;
	HIP_TRY(c, hipEventSynchronize(ev.end));
	HIP_TRY(c, hipEventElapsedTime(&f, ev.begin, ev.end));
	*ms = f;
	return FSEQ_OK;
}

// The distinct long-path lengths, ascending.  The first is a base: phases A and B, the capacity estimate, and the ordinary attempts
// up to their verdict.  Every further length folds the lists of the length before it and runs the DP alone; where the DP flags a
// cell unproven -- and under list windows or FSEQ_SCAN_REBUILD always -- that length becomes a new base: the lists are built at it by
// the ordinary attempts, from the capacity in force on.
int scan_long(fseq_ctx *c, ScanPlan const &P, std::vector<ScanSlot> &slots, fseq_length_scan_summary &sum, ScanEvents const &ev)
{
	hipStream_t st = c->stream;
	int rc;
	LongRun R;
	for (size_t i = 0; i < P.long_lengths.size(); ++i)
	{
		if ((rc = apply_segment_length(c, P.long_lengths[i]))) return rc;
		ScanSlot &s = slots[i];
		if (i == 0)
		{
			R.X = c->p.list_cap ? c->p.list_cap : FSEQ_X_FLOOR;
			c->tm = fseq_timings{};
			if ((rc = ensure_work_buffers(c, 0))) return rc;
			auto close_ab = [&](int code) { if (R.range_ab_open) { FSEQ_RANGE_POP(); R.range_ab_open = false; } return code; };
			if ((rc = long_phase_a(c, R))) return close_ab(rc);
			if ((rc = long_phase_b(c, R))) return close_ab(rc);
			if ((rc = long_list_capacity(c, R))) return rc;
		}
		HIP_TRY(c, hipEventRecord(ev.begin, st));
		// (no whole list set to fold under list windows: the verdict of the entry before says whether its lists were windowed)
		bool build = i == 0 || c->tune.scan_rebuild || c->lw.on;
		DpProof proof;
		if (!build)
		{
			RelumpArgs A;
			A.lists = list_args(c); A.k0 = 0; A.ncols = c->p.n;
			launch_relump_lists(st, A);
			HIP_TRY(c, hipGetLastError());
			bool unproven = false;
			if ((rc = long_dp_on_lists(c, &proof, &unproven))) return rc;
			build = unproven;
			if (unproven && c->tune.debug)
				fprintf(stderr, "[fseq] length scan: the folded lists do not prove L = %llu: built at this length\n", (unsigned long long) P.long_lengths[i]);
		}
		s.lists = build ? FSEQ_SCAN_LISTS_BUILT : FSEQ_SCAN_LISTS_FOLDED;
		if (build)
		{
			c->red.memory.forget_input();                         // (the representatives' plan and marks are of another length)
			if ((rc = long_attempts_to_proof(c, R, &proof))) return rc;
		}
		HIP_TRY(c, hipEventRecord(ev.end, st));
		if ((rc = scan_elapsed(c, ev, &s.ms))) return rc;
		s.max_segment_size = proof.max_segment_size;
		s.list_cap = c->X;
		s.dp_chunks = proof.dp_chunks;
		++(build ? sum.lists_built : sum.lists_folded);
	}
	sum.retries = R.retries;
	float f = 0;
	HIP_TRY(c, hipEventElapsedTime(&f, c->ev.a_begin, c->ev.a_end_b_begin)); sum.ms_phase_a = f;
	HIP_TRY(c, hipEventElapsedTime(&f, c->ev.a_end_b_begin, c->ev.b_end)); sum.ms_phase_b = f;
	return FSEQ_OK;
}

// the scan between its refusals and the restoring of the context's own state
int scan_body(fseq_ctx *c, ScanPlan const &P, std::vector<ScanSlot> &slots, ScanSlot &short_slot, fseq_length_scan_summary &sum)
{
	int rc;
	ScanEvents ev;
	HIP_TRY(c, hipEventCreate(&ev.begin));
	HIP_TRY(c, hipEventCreate(&ev.end));
	if (!c->kernels_ready && (rc = prepare_geometry(c))) return rc;
	if (!P.long_lengths.empty() && (rc = scan_long(c, P, slots, sum, ev))) return rc;
	if (P.n_short)
	{
		// segmentation_sp_context: the distinct rows of [0, n), whatever the length
		fseq_result r{};
		HIP_TRY(c, hipEventRecord(ev.begin, c->stream));
		rc = run_short_path(c, &r);
		if (rc && rc != FSEQ_E_NO_REDUCTION) return rc;
		HIP_TRY(c, hipEventRecord(ev.end, c->stream));
		if ((rc = scan_elapsed(c, ev, &short_slot.ms))) return rc;
		short_slot.max_segment_size = r.max_segment_size;
		short_slot.lists = FSEQ_SCAN_LISTS_NONE;
	}
	return FSEQ_OK;
}

// the device arrays of one debug call: freed when the call returns, whichever way
struct RelumpBuffers {
	void *ent = nullptr, *hdr = nullptr;
	~RelumpBuffers() { if (ent) (void) hipFree(ent); if (hdr) (void) hipFree(hdr); }
};

} // namespace

} // namespace fseq

using namespace fseq;

extern "C" {

int fseq_set_segment_length(fseq_ctx *c, uint64_t segment_length)
{
	if (!c) return FSEQ_E_ARG;
	if (0 == segment_length) return fail(c, FSEQ_E_ARG, "the segment length must be positive");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "a sharded context keeps its segment length: its block geometry and halo depend on it");
	if (c->in.open) return fail(c, FSEQ_E_ARG, "a chunked input is under way (fseq_input_begin without fseq_input_end)");
	(void) hipSetDevice(c->p.device);
	if (c->stream) (void) hipStreamSynchronize(c->stream);
	uint64_t const before = c->p.segment_length;
	if (int const rc = apply_segment_length(c, segment_length))
	{
		(void) apply_segment_length(c, before);                   // (the work buffers are gone: nothing is allocated here)
		return rc;
	}
	// the result and the last match go, as behind a new input; so does what runs learnt that depends on the length
	c->have_result = false;
	c->scan_lists = false;
	c->free_match();
	c->red.memory.forget_input();
	c->X_hint = 0;
	c->tb_guess = 0;
	return FSEQ_OK;
}

int fseq_scan_segment_lengths(fseq_ctx *c, fseq_length_scan_entry *entries, size_t count, fseq_length_scan_summary *summary)
{
	if (!c) return FSEQ_E_ARG;
	if (!entries || !summary || 0 == count) return fail(c, FSEQ_E_ARG, "length scan: entries, a count and a summary are needed");
	if (count > 0xFFFFFFFFull) return fail(c, FSEQ_E_ARG, "length scan: too many entries");
	std::vector<uint64_t> lengths(count);
	for (size_t i = 0; i < count; ++i)
	{
		lengths[i] = entries[i].segment_length;
		if (0 == lengths[i]) return fail(c, FSEQ_E_ARG, "length scan: a segment length must be positive");
	}
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "length scan: not for sharded contexts (their block geometry and halo depend on the segment length)");
	if (!c->have_input) return fail(c, FSEQ_E_ARG, "no input set");
	(void) hipSetDevice(c->p.device);
	double const t_begin = now_ms();
	ScanPlan const P = plan_length_scan(c->p.n, lengths.data(), count);
	std::vector<ScanSlot> slots(P.long_lengths.size());
	ScanSlot short_slot;
	fseq_length_scan_summary sum{};
	// the context holds no result from here on; its own length and what its runs learnt at that length come back behind the scan
	uint64_t const own_length = c->p.segment_length;
	uint32_t const own_X_hint = c->X_hint;
	c->have_result = false;
	c->scan_lists = false;
	c->free_match();
	c->lw.on = false; c->lw.merge_windows = 0;
	c->X_hint = 0;
	c->red.memory.forget_input();
	int rc = scan_body(c, P, slots, short_slot, sum);
	bool const lists_held = rc == FSEQ_OK && !P.long_lengths.empty();
	c->have_result = false;                                       // (the short path's sweep leaves one)
	c->X_hint = own_X_hint;
	c->red.memory.forget_input();
	int const rc_back = apply_segment_length(c, own_length);
	if (!rc) rc = rc_back;
	if (rc) return rc;
	c->scan_lists = lists_held && c->d_ent;                       // fseq_debug_column_list: the lists of the last long-path entry
	sum.short_entries = P.n_short;
	sum.ms_total = now_ms() - t_begin;
	std::vector<uint8_t> seen(slots.size(), 0);
	bool short_seen = false;
	for (size_t i = 0; i < count; ++i)
	{
		fseq_length_scan_entry &e = entries[i];
		bool const is_short = P.slot[i] < 0;
		ScanSlot const &s = is_short ? short_slot : slots[(size_t) P.slot[i]];
		bool const first = is_short ? !short_seen : !seen[(size_t) P.slot[i]];
		if (is_short) short_seen = true; else seen[(size_t) P.slot[i]] = 1;
		e.max_segment_size = s.max_segment_size;
		e.short_path = is_short ? 1u : 0u;
		e.lists = s.lists;
		e.list_cap = is_short ? 0u : s.list_cap;
		e.dp_chunks = is_short ? 0u : s.dp_chunks;
		e.reserved = 0;
		e.ms_device = first ? s.ms : 0.0;
	}
	*summary = sum;
	return FSEQ_OK;
}

int fseq_debug_scan_plan(uint64_t n, uint64_t const *lengths, uint32_t count, uint64_t *long_lengths, uint32_t *n_long, int32_t *slot, uint32_t *n_short)
{
	if (!lengths || !long_lengths || !n_long || !slot || !n_short || 0 == count || 0 == n) return FSEQ_E_ARG;
	for (uint32_t i = 0; i < count; ++i)
		if (0 == lengths[i]) return FSEQ_E_ARG;
	ScanPlan const P = plan_length_scan(n, lengths, count);
	std::copy(P.long_lengths.begin(), P.long_lengths.end(), long_lengths);
	std::copy(P.slot.begin(), P.slot.end(), slot);
	*n_long = (uint32_t) P.long_lengths.size();
	*n_short = P.n_short;
	return FSEQ_OK;
}

int fseq_debug_relump_lists(int device, uint64_t k0, uint32_t ncols, uint32_t stride, uint64_t L_from, uint64_t L_to, uint32_t *ent, uint32_t *hdr)
{
	// ---- everything the kernel forms an index from, before the first HIP call
	if (!ent || !hdr || 0 == ncols || 0 == stride || 0 == L_from || L_to < L_from || L_to > 0xFFFFFFFFull) return FSEQ_E_ARG;
	if (k0 + ncols > (1ull << 32) || (uint64_t) ncols * stride > (1ull << 28)) return FSEQ_E_ARG;
	for (uint32_t j = 0; j < ncols; ++j)
		if (0 == hdr[4 * (size_t) j] || hdr[4 * (size_t) j] > stride) return FSEQ_E_ARG;
	if (hipSetDevice(device) != hipSuccess) return FSEQ_E_HIP;
	RelumpBuffers B;
	size_t const ent_bytes = (size_t) ncols * stride * sizeof(uint2), hdr_bytes = (size_t) ncols * sizeof(uint4);
	if (hipMalloc(&B.ent, ent_bytes) != hipSuccess || hipMalloc(&B.hdr, hdr_bytes) != hipSuccess) { (void) hipGetLastError(); return FSEQ_E_OOM; }
	if (hipMemcpy(B.ent, ent, ent_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(B.hdr, hdr, hdr_bytes, hipMemcpyHostToDevice) != hipSuccess) return FSEQ_E_HIP;
	// (the kernel addresses a column by its place in the alignment, as the context's rebased buffers are: column k0 is the arrays' first)
	RelumpArgs A;
	A.lists.L = (uint32_t) L_to; A.lists.stride = stride;
	A.lists.ent = reinterpret_cast<uint2 *>(reinterpret_cast<uintptr_t>(B.ent) - (uintptr_t) (k0 * stride * sizeof(uint2)));
	A.lists.hdr = reinterpret_cast<uint4 *>(reinterpret_cast<uintptr_t>(B.hdr) - (uintptr_t) (k0 * sizeof(uint4)));
	A.k0 = k0; A.ncols = ncols;
	launch_relump_lists(nullptr, A);
	if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FSEQ_E_HIP;
	if (hipMemcpy(ent, B.ent, ent_bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hdr, B.hdr, hdr_bytes, hipMemcpyDeviceToHost) != hipSuccess) return FSEQ_E_HIP;
	return FSEQ_OK;
}

} // extern "C"
