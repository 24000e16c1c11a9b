// fseq_api_rowsplit.hip -- the part of the C ABI (include/fseq.h) that makes a context over some rows of the resident alignment
// and keeps the others aside, packed, for fseq_match_held_out (csrc/fseq_api_match.hip): leave-rows-out validation without a
// second upload.
//
// replaces: nothing of the reference, where rows are held out by removing their lines from the list file; the new context's results
// are what its chain produces from that shorter file.  The plan is csrc/fseq_rowsplit_plan.hpp (host only), the kernel
// csrc/fseq_rowsplit.hpp.  A translation unit of its own: nothing here is allocated or launched unless its entry points are
// called, and nothing of the source context's segmentation state is read or written.
#include "fseq_ctx.hpp"
#include "fseq_rowsplit.hpp"

using namespace fseq;

namespace {

struct Events {
	hipEvent_t ev[2]{};
	hipError_t create()
	{
		for (auto &e : ev)
		{
			hipError_t const rc = hipEventCreate(&e);
			if (rc != hipSuccess) { e = nullptr; return rc; }
		}
		return hipSuccess;
	}
	~Events() { for (auto &e : ev) if (e) (void) hipEventDestroy(e); }
};

int refuse(fseq_ctx *c, char const *why)
{
	char what[256];
	snprintf(what, sizeof(what), "without rows: %s", why);
	return fail(c, FSEQ_E_ARG, what);
}

void launch_split(hipStream_t st, uint32_t bits, dim3 grid, RowSplitArgs const &A)
{
	switch (bits)
	{
		case 2: hipLaunchKernelGGL(k_rows_split<2>, grid, dim3(RS_T), rs_lds_bytes(A), st, A); break;
		case 4: hipLaunchKernelGGL(k_rows_split<4>, grid, dim3(RS_T), rs_lds_bytes(A), st, A); break;
		default: hipLaunchKernelGGL(k_rows_split<8>, grid, dim3(RS_T), rs_lds_bytes(A), st, A); break;
	}
}

} // namespace

extern "C" {

int fseq_create_without_rows(fseq_ctx *src, uint32_t const *held_rows, uint32_t n_held, fseq_params const *params, fseq_ctx **out, fseq_hold_out_summary *summary)
{
	if (!params || !out) return FSEQ_E_ARG;
	*out = nullptr;
	if (!src) return FSEQ_E_ARG;
	fseq_ctx *const c = src;
	if (!held_rows) return refuse(c, "no list of held-out rows");
	if (params->m != 0) return refuse(c, "params->m must be 0 (it becomes the number of kept rows)");
	if (params->n != 0 && params->n != c->p.n) return refuse(c, "params->n must be 0 or the source's");
	if (params->device != c->p.device) return refuse(c, "params->device must be the source's device");
	if (0 == params->segment_length) return refuse(c, "params->segment_length must be positive");
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "without rows: sharded context: a rank holds its own columns only");
	if (c->idn.have) return fail(c, FSEQ_E_UNSUPPORTED, "without rows: the source was made by fseq_create_without_identity_columns (its identity state would have to be carried along; hold the rows out first)");
	if (!c->have_input || !c->d_msa) return refuse(c, "no alignment resident on the device");
	uint32_t const m = c->p.m, bits = 8u >> c->bsh;
	uint64_t const n = c->p.n;
	RowSplitPlan P;
	RowSplitStrips S;
	std::vector<uint2> desc;
	try
	{
		if (char const *why = row_split_refuse(m, bits, held_rows, n_held)) return refuse(c, why);
		P = row_split_plan(m, bits, held_rows, n_held);
		S = row_split_strips(m, bits, P);
		desc.assign((size_t) 4u * S.out_chunks, make_uint2(RS_PAD_WORD, 0u));
		for (uint32_t w = 0; w < P.n_words; ++w) desc[w] = make_uint2(P.base[w], P.keep[w]);
	}
	catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "without rows: the plan (host)"); }
	uint32_t const kept = (uint32_t) P.kept.size();

	// --- from here on a device is touched ---
	(void) hipSetDevice(c->p.device);
	hipStream_t const st = c->stream;
	Events E;
	HIP_TRY(c, E.create());
	DevTemp<uint2> d_desc(c);
	DevTemp<uint32_t> d_kept(c), d_held(c);
	DevTemp<RowSplitStrip> d_strips(c);
	int rc;
	if ((rc = d_desc.alloc(desc.size())) || (rc = d_kept.alloc(kept)) || (rc = d_held.alloc(n_held)) || (rc = d_strips.alloc(S.strips.size()))) return rc;

	// the new context: an ordinary one over the kept rows, with the source's alphabet, codes and packing as they are
	fseq_params p = *params;
	p.m = kept;
	p.n = n;
	fseq_ctx *d = nullptr;
	if ((rc = fseq_create(&p, &d))) return fail(c, rc, "without rows: fseq_create of the new context failed");
	d->sigma = c->sigma;
	memcpy(d->code_to_byte, c->code_to_byte, sizeof(d->code_to_byte));
	d->bsh = c->bsh;                                       // (not from sigma: a borrowed one-byte-per-code source keeps its width)
	d->ld = (size_t) S.out_chunks * 16u;
	size_t const h_bytes = ((size_t) n_held * bits + 7u) / 8u, ld_h = (h_bytes + 15u) & ~size_t(15);
	try { d->hold.kept_rows = std::move(P.kept); d->hold.held_rows.assign(held_rows, held_rows + n_held); }
	catch (std::bad_alloc const &) { fseq_destroy(d); return fail(c, FSEQ_E_OOM, "without rows: the row maps (host)"); }
	if ((rc = d->d_msa_own.alloc(d, d->ld * (size_t) n + 16)) || (rc = d->hold.cols.alloc(d, ld_h * (size_t) n + 16)))
	{
		char what[400];
		snprintf(what, sizeof(what), "without rows: %llu columns of %zu bytes for the kept rows and of %zu bytes for the held-out rows: %s",
		         (unsigned long long) n, d->ld, ld_h, d->err.c_str());
		fseq_destroy(d);
		return fail(c, rc, what);
	}
	d->d_msa = d->d_msa_own.base;
	auto give_up = [&](char const *what, hipError_t e) { (void) hipStreamSynchronize(st); fseq_destroy(d); return fail(c, FSEQ_E_HIP, what, e); };
	hipError_t e;
	if ((e = hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(uint2), hipMemcpyHostToDevice, st)) != hipSuccess) return give_up("without rows: descriptors", e);
	if ((e = hipMemcpyAsync(d_kept, d->hold.kept_rows.data(), (size_t) kept * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return give_up("without rows: kept rows", e);
	if ((e = hipMemcpyAsync(d_held, held_rows, (size_t) n_held * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return give_up("without rows: held rows", e);
	if ((e = hipMemcpyAsync(d_strips, S.strips.data(), S.strips.size() * sizeof(RowSplitStrip), hipMemcpyHostToDevice, st)) != hipSuccess) return give_up("without rows: strips", e);
	RowSplitArgs A{};
	A.src = c->d_msa; A.src_ld = c->ld; A.n = n;
	A.desc = d_desc; A.kept = d_kept; A.n_kept = kept; A.held = d_held; A.n_held = n_held;
	A.strips = d_strips; A.whole = S.whole ? 1u : 0u; A.tile_cols = S.tile_cols;
	for (RowSplitStrip const &s_ : S.strips)
	{
		A.lds_in = std::max(A.lds_in, S.tile_cols * (s_.src_chunks + 1u));
		A.lds_out = std::max(A.lds_out, S.tile_cols * (s_.c1 - s_.c0));
		A.lds_desc = std::max(A.lds_desc, 4u * (s_.c1 - s_.c0));
	}
	A.dst = d->d_msa; A.dst_ld = d->ld; A.hdst = d->hold.cols; A.h_ld = ld_h;
	uint32_t const ns = (uint32_t) S.strips.size();
	uint64_t const tiles = (n + S.tile_cols - 1u) / S.tile_cols;
	dim3 const grid((uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::max(1u, 8192u / ns))), ns);
	if ((e = hipEventRecord(E.ev[0], st)) != hipSuccess) return give_up("without rows: event", e);
	launch_split(st, bits, grid, A);
	if ((e = hipGetLastError()) != hipSuccess) return give_up("without rows: launch", e);
	if ((e = hipEventRecord(E.ev[1], st)) != hipSuccess) return give_up("without rows: event", e);
	if ((e = hipStreamSynchronize(st)) != hipSuccess) return give_up("without rows: the split", e);
	float ms = 0.f;
	(void) hipEventElapsedTime(&ms, E.ev[0], E.ev[1]);
	d->hold.have = true;
	d->hold.m_src = m;
	d->hold.n_held = n_held;
	d->hold.ld = ld_h;
	d->have_input = true;
	if (summary) *summary = fseq_hold_out_summary{m, n_held, kept, 0u, (double) ms};
	*out = d;
	return FSEQ_OK;
}

int fseq_get_held_out(fseq_ctx *c, uint32_t *kept_rows, uint32_t *held_rows)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->hold.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	if (kept_rows) std::copy(c->hold.kept_rows.begin(), c->hold.kept_rows.end(), kept_rows);
	if (held_rows) std::copy(c->hold.held_rows.begin(), c->hold.held_rows.end(), held_rows);
	return FSEQ_OK;
}

int fseq_debug_held_out_columns(fseq_ctx *c, uint64_t c0, uint64_t c1, uint8_t *out, uint64_t *ld, uint32_t *bits)
{
	if (!c || !ld || !bits) return FSEQ_E_ARG;
	if (!c->hold.have) return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_rows");
	if (c0 > c1 || c1 > c->p.n) return fail(c, FSEQ_E_ARG, "held-out columns: columns out of range");
	*ld = c->hold.ld;
	*bits = 8u >> c->bsh;
	if (!out || c0 == c1) return FSEQ_OK;
	(void) hipSetDevice(c->p.device);
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(out, c->hold.cols + (size_t) c0 * c->hold.ld, (size_t) (c1 - c0) * c->hold.ld, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

int fseq_debug_row_split_plan(uint32_t m, uint32_t bits, uint32_t const *held, uint32_t n_held, uint32_t *kept, uint32_t *base, uint32_t *keep,
                              uint32_t *n_words, uint32_t *n_slow)
{
	if (!n_words || !n_slow) return FSEQ_E_ARG;
	try
	{
		if (row_split_refuse(m, bits, held, n_held)) return FSEQ_E_ARG;
		RowSplitPlan const P = row_split_plan(m, bits, held, n_held);
		if (kept) std::copy(P.kept.begin(), P.kept.end(), kept);
		if (base) std::copy(P.base.begin(), P.base.end(), base);
		if (keep) std::copy(P.keep.begin(), P.keep.end(), keep);
		*n_words = P.n_words;
		*n_slow = P.n_slow;
	}
	catch (std::bad_alloc const &) { return FSEQ_E_OOM; }
	return FSEQ_OK;
}

} // extern "C"
