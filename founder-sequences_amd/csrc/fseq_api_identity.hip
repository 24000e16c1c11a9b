// fseq_api_identity.hip -- the part of the C ABI (include/fseq.h) that finds the identity columns of the resident alignment,
// makes a context over the other columns and writes that context's founders with the identity columns put back.
//
// replaces: remove-identity-columns (main.cc:105-153, :157-227) in front of founder_sequences and insert-identity-columns
// (main.cc:138-195) behind it, which go through m reduced files and read the founders back.  The kernels are in
// fseq_identity.hpp.  A translation unit of its own: nothing here is allocated or launched unless its entry points are
// called, and nothing of the source context's segmentation state is touched.
#include "fseq_ctx.hpp"
#include "fseq_identity.hpp"
#include "fseq_exceptions.hpp"

using namespace fseq;

namespace {

struct Events {
	hipEvent_t ev[4]{};
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

int refuse_source(fseq_ctx *c)
{
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "identity columns: sharded context: a rank holds its own columns only");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "identity columns: no alignment resident on the device");
	return FSEQ_OK;
}

uint32_t grid_for(uint64_t groups) { return (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(groups, 16384)); }

// the mask pass on c's stream: d_mask[n], *d_count += identity columns (d_count zeroed here)
int launch_mask(fseq_ctx *c, IdShape const &s, uint8_t *d_mask, uint32_t *d_count)
{
	HIP_TRY(c, hipMemsetAsync(d_count, 0, 4, c->stream));
	uint64_t const groups = (c->p.n + s.cols_per_wg - 1u) / s.cols_per_wg;
	hipLaunchKernelGGL(k_identity_mask, dim3(grid_for(groups)), dim3(ID_T), 0, c->stream, c->d_msa, c->ld, (uint64_t) c->p.n, c->bsh, s, d_mask, d_count);
	HIP_TRY(c, hipGetLastError());
	return FSEQ_OK;
}

int not_reduced(fseq_ctx *c) { return fail(c, FSEQ_E_ARG, "not a context made by fseq_create_without_identity_columns"); }

} // namespace

extern "C" {

int fseq_identity_columns(fseq_ctx *c, uint8_t *mask, fseq_identity_summary *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	int rc = refuse_source(c);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	uint64_t const n = c->p.n;
	IdShape const s = id_shape(c->p.m, c->bsh);
	DevTemp<uint8_t> d_mask(c);
	DevTemp<uint32_t> d_count(c);
	if ((rc = d_mask.alloc((size_t) n)) || (rc = d_count.alloc(1))) return rc;
	Events E;
	HIP_TRY(c, E.create());
	HIP_TRY(c, hipEventRecord(E.ev[0], c->stream));
	if ((rc = launch_mask(c, s, d_mask, d_count))) return rc;
	HIP_TRY(c, hipEventRecord(E.ev[1], c->stream));
	uint32_t identity = 0;
	HIP_TRY(c, hipMemcpyAsync(&identity, d_count, 4, hipMemcpyDeviceToHost, c->stream));
	if (mask) HIP_TRY(c, hipMemcpyAsync(mask, d_mask, (size_t) n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipGetLastError());
	float ms = 0.f;
	HIP_TRY(c, hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
	*out = fseq_identity_summary{n, identity, n - identity, (double) ms};
	return FSEQ_OK;
}

// fseq_create_without_identity_columns and -- held -- fseq_create_without_identity_columns_held, which carries the held-out rows
// of a source made by fseq_create_without_rows along: their kept columns, the two row maps and their exception cells
static int create_without_identity_columns(fseq_ctx *src, fseq_params const *params, fseq_ctx **out, fseq_identity_summary *summary, bool held)
{
	if (!params || !out) return FSEQ_E_ARG;
	*out = nullptr;
	if (params->n != 0) return src ? fail(src, FSEQ_E_ARG, "without identity columns: params->n must be 0 (it becomes the number of kept columns)") : FSEQ_E_ARG;
	if (!src) return FSEQ_E_ARG;
	fseq_ctx *const c = src;
	if (held && (!c->hold.have || c->idn.have)) return fail(c, FSEQ_E_ARG, "without identity columns, held-out rows kept: the source is not a context made by fseq_create_without_rows");
	if (params->m != 0 && params->m != c->p.m) return fail(c, FSEQ_E_ARG, "without identity columns: params->m must be 0 or the source's");
	if (params->device != c->p.device) return fail(c, FSEQ_E_ARG, "without identity columns: params->device must be the source's device");
	if (0 == params->segment_length) return fail(c, FSEQ_E_ARG, "without identity columns: params->segment_length must be positive");
	int rc = refuse_source(c);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	hipStream_t const st = c->stream;
	uint64_t const n = c->p.n;
	uint32_t const ntiles = (uint32_t) ((n + ID_TILE - 1u) / ID_TILE);
	IdShape const s = id_shape(c->p.m, c->bsh);
	Events E;
	HIP_TRY(c, E.create());

	// the mask and the scan of its tiles, in buffers of this call: nothing exists yet when every column turns out to be one
	DevTemp<uint8_t> d_mask(c), d_lut(c);
	DevTemp<uint32_t> d_count(c), d_tiles(c);
	if ((rc = d_mask.alloc((size_t) n)) || (rc = d_count.alloc(1)) || (rc = d_tiles.alloc((size_t) ntiles + 1)) || (rc = d_lut.alloc(256))) return rc;
	HIP_TRY(c, hipEventRecord(E.ev[0], st));
	if ((rc = launch_mask(c, s, d_mask, d_count))) return rc;
	hipLaunchKernelGGL(k_identity_count, dim3(ntiles), dim3(ID_T), 0, st, d_mask, n, d_tiles);
	hipLaunchKernelGGL(k_identity_offsets, dim3(1), dim3(ID_T), 0, st, d_tiles, ntiles);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(E.ev[1], st));
	uint32_t identity = 0, kept32 = 0;
	HIP_TRY(c, hipMemcpyAsync(&identity, d_count, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(&kept32, d_tiles + ntiles, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(d_lut, c->code_to_byte, 256, hipMemcpyHostToDevice, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	HIP_TRY(c, hipGetLastError());
	uint64_t const kept = kept32;
	if (identity + kept != n) return fail(c, FSEQ_E_HIP, "identity columns: the mask pass and the scan disagree");
	if (0 == kept) return fail(c, FSEQ_E_ARG, "every column is an identity column: nothing is left to segment");

	// the new context: an ordinary one over the kept columns, with the source's alphabet, codes and packing as they are
	fseq_params p = *params;
	p.m = c->p.m;
	p.n = kept;
	fseq_ctx *d = nullptr;
	if ((rc = fseq_create(&p, &d))) return fail(c, rc, "without identity columns: fseq_create of the new context failed");
	d->sigma = c->sigma;
	memcpy(d->code_to_byte, c->code_to_byte, sizeof(d->code_to_byte));
	d->bsh = c->bsh;                                       // (not from sigma: a borrowed one-byte-per-code source keeps its width)
	d->ld = (size_t) s.chunks * 16u;
	d->idn.n_src = n;
	d->idn.identity = identity;
	if ((rc = d->d_msa_own.alloc(d, d->ld * (size_t) kept + 16)) || (rc = d->idn.mask.alloc(d, (size_t) n)) || (rc = d->idn.kept.alloc(d, (size_t) kept)) ||
	    (rc = d->idn.ref.alloc(d, (size_t) n)))
	{
		char what[400];
		snprintf(what, sizeof(what), "without identity columns: %llu kept columns of %zu bytes, a mask and a reference of %llu bytes each, %llu column indices: %s",
		         (unsigned long long) kept, d->ld, (unsigned long long) n, (unsigned long long) kept, d->err.c_str());
		fseq_destroy(d);
		return fail(c, rc, what);
	}
	d->d_msa = d->d_msa_own.base;
	auto give_up = [&](char const *what, hipError_t e) { (void) hipStreamSynchronize(st); fseq_destroy(d); return fail(c, FSEQ_E_HIP, what, e); };
	hipError_t e;
	if ((e = hipEventRecord(E.ev[2], st)) != hipSuccess) return give_up("without identity columns: event", e);
	if ((e = hipMemcpyAsync(d->idn.mask, d_mask, (size_t) n, hipMemcpyDeviceToDevice, st)) != hipSuccess) return give_up("without identity columns: mask copy", e);
	hipLaunchKernelGGL(k_identity_scatter, dim3(ntiles), dim3(ID_T), 0, st, d_mask, n, d_tiles, d->idn.kept);
	uint32_t const cols_per_wg = std::max<uint32_t>(1u, 4096u / s.chunks);
	hipLaunchKernelGGL(k_identity_gather, dim3(grid_for((kept + cols_per_wg - 1u) / cols_per_wg)), dim3(ID_T), 0, st, c->d_msa, c->ld, d->idn.kept, kept, c->bsh, s,
	                   cols_per_wg, d->d_msa);
	hipLaunchKernelGGL(k_identity_ref, dim3(grid_for((n + ID_T - 1u) / ID_T)), dim3(ID_T), 0, st, c->d_msa, c->ld, n, c->bsh, d_lut, d->idn.ref);
	if ((e = hipGetLastError()) != hipSuccess) return give_up("without identity columns: scatter / gather launch", e);
	if ((e = hipEventRecord(E.ev[3], st)) != hipSuccess) return give_up("without identity columns: event", e);
	if ((e = hipStreamSynchronize(st)) != hipSuccess) return give_up("without identity columns: scatter / gather", e);
	float ms0 = 0.f, ms1 = 0.f;
	(void) hipEventElapsedTime(&ms0, E.ev[0], E.ev[1]);
	(void) hipEventElapsedTime(&ms1, E.ev[2], E.ev[3]);
	if (held)
	{
		// the held-out rows: their kept columns gathered as the alignment's were, and the identity columns in which one of them
		// differs from row 0 marked in a bit matrix of this call, from which the lists are made (csrc/fseq_exceptions.hpp)
		auto carry = [&]() -> int {
			auto &H = d->hold;
			uint32_t const n_held = c->hold.n_held;
			IdShape const hs = id_shape(n_held, c->bsh);                  // (chunks * 16 is the source's hold.ld)
			size_t const ld_h = (size_t) hs.chunks * 16u, nw = (size_t) ((n + 31u) / 32u);
			try { H.kept_rows = c->hold.kept_rows; H.held_rows = c->hold.held_rows; }
			catch (std::bad_alloc const &) { return fail(d, FSEQ_E_OOM, "the row maps (host)"); }
			DevTemp<uint32_t> d_bits(d);
			int rc2;
			if ((rc2 = H.cols.alloc(d, ld_h * (size_t) kept + 16)) || (rc2 = d_bits.alloc((size_t) n_held * nw))) return rc2;
			HIP_TRY(d, hipMemsetAsync(d_bits, 0, (size_t) n_held * nw * 4, st));
			uint32_t const hcols_per_wg = std::max<uint32_t>(1u, 4096u / hs.chunks);
			hipLaunchKernelGGL(k_identity_gather, dim3(grid_for((kept + hcols_per_wg - 1u) / hcols_per_wg)), dim3(ID_T), 0, st, (uint8_t const *) c->hold.cols, c->hold.ld,
			                   (uint32_t const *) d->idn.kept, kept, c->bsh, hs, hcols_per_wg, (uint8_t *) H.cols);
			hipLaunchKernelGGL(k_exc_bits_held, dim3(grid_for((n * hs.chunks + EX_T - 1u) / EX_T)), dim3(EX_T), 0, st, (uint8_t const *) c->hold.cols, c->hold.ld, n_held,
			                   hs.chunks, (uint8_t const *) c->d_msa, c->ld, (uint8_t const *) d->idn.mask, n, c->bsh, (uint32_t *) d_bits, nw);
			HIP_TRY(d, hipGetLastError());
			if ((rc2 = exc_lists_from_bits(d, st, d_bits, nw, n_held, H.exc_off, H.exc_cols, &H.exc_total))) return rc2;
			H.have = H.have_exc = true;
			H.m_src = c->hold.m_src;
			H.n_held = n_held;
			H.ld = ld_h;
			return FSEQ_OK;
		};
		if ((rc = carry()))
		{
			char what[400];
			snprintf(what, sizeof(what), "without identity columns, held-out rows kept: %u held-out rows over %llu kept and %llu source columns: %s",
			         c->hold.n_held, (unsigned long long) kept, (unsigned long long) n, d->err.c_str());
			(void) hipStreamSynchronize(st);
			fseq_destroy(d);
			return fail(c, rc, what);
		}
	}
	d->idn.have = true;
	d->have_input = true;
	if (summary) *summary = fseq_identity_summary{n, identity, kept, (double) ms0 + (double) ms1};
	*out = d;
	return FSEQ_OK;
}

int fseq_create_without_identity_columns(fseq_ctx *src, fseq_params const *params, fseq_ctx **out, fseq_identity_summary *summary)
{
	return create_without_identity_columns(src, params, out, summary, false);
}

int fseq_create_without_identity_columns_held(fseq_ctx *src, fseq_params const *params, fseq_ctx **out, fseq_identity_summary *summary)
{
	return create_without_identity_columns(src, params, out, summary, true);
}

int fseq_get_identity_columns(fseq_ctx *c, uint8_t *mask, uint64_t *kept_columns)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->idn.have) return not_reduced(c);
	(void) hipSetDevice(c->p.device);
	if (mask) HIP_TRY(c, hipMemcpy(mask, c->idn.mask, (size_t) c->idn.n_src, hipMemcpyDeviceToHost));
	if (kept_columns)
	{
		std::vector<uint32_t> k32;
		try { k32.resize((size_t) c->p.n); } catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "kept-column list (host)"); }
		HIP_TRY(c, hipMemcpy(k32.data(), c->idn.kept, k32.size() * 4, hipMemcpyDeviceToHost));
		for (size_t j = 0; j < k32.size(); ++j) kept_columns[j] = k32[j];
	}
	return FSEQ_OK;
}

int fseq_write_identity_columns(fseq_ctx *c, char const *path)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->idn.have) return not_reduced(c);
	std::vector<uint8_t> text;
	try { text.resize((size_t) c->idn.n_src + 1); } catch (std::bad_alloc const &) { return fail(c, FSEQ_E_OOM, "identity-column text (host)"); }
	int const rc = fseq_get_identity_columns(c, text.data(), nullptr);
	if (rc) return rc;
	for (size_t k = 0; k + 1 < text.size(); ++k) text[k] = text[k] ? '1' : '0';     // remove-identity-columns/main.cc:139-146
	text.back() = '\n';                                                             // main.cc:225
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the identity-columns output file");
	bool const ok = fwrite(text.data(), 1, text.size(), f) == text.size();
	fflush(f);
	if (f != stdout) fclose(f);
	if (!ok) return fail(c, FSEQ_E_ARG, "writing the identity-columns output file failed");
	return FSEQ_OK;
}

// fseq_write_founders_device's batches (csrc/fseq_api_join.hip) with lines of the source's length: a batch is filled with the
// reference bytes, then the kept positions are written over them
int fseq_write_founders_restored(fseq_ctx *c, uint32_t const *permutations, char const *path)
{
	if (!c || !permutations) return FSEQ_E_ARG;
	if (!c->idn.have) return not_reduced(c);
	if (!c->have_result || c->res.short_path) return fail(c, FSEQ_E_ARG, "restored founders need a finished long-path run (short path: the founders are input rows)");
	if (!c->have_input || !c->d_msa) return fail(c, FSEQ_E_ARG, "no alignment resident on the device");
	(void) hipSetDevice(c->p.device);
	size_t const X = c->res.max_segment_size, S = c->segments.size();
	if (!X || !S) return fail(c, FSEQ_E_ARG, "no segments to write");
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) return fail(c, FSEQ_E_ARG, "cannot open the founders output file");
	hipStream_t st = c->stream;
	uint64_t const n_src = c->idn.n_src;
	size_t const line = (size_t) n_src + 1;
	size_t const batch = std::max<size_t>(1, std::min<size_t>(X, (size_t) (256u << 20) / line));
	size_t const bytes = (batch * line + 15) & ~size_t(15);
	DevTemp<uint32_t> d_perm(c);
	DevTemp<uint64_t> d_seg(c);
	DevTemp<uint8_t> d_lut(c), d_out(c);
	uint8_t *h_out = nullptr;
	int rc = FSEQ_OK;
	auto cleanup = [&]() {
		if (h_out) (void) hipHostFree(h_out);
		if (f != stdout) fclose(f);
	};
	if ((rc = d_perm.alloc(S * X)) || (rc = d_seg.alloc(2 * S)) || (rc = d_lut.alloc(256)) || (rc = d_out.alloc(bytes))) { cleanup(); return rc; }
	if (hipHostMalloc(reinterpret_cast<void **>(&h_out), bytes, hipHostMallocDefault) != hipSuccess) { h_out = nullptr; (void) hipGetLastError(); cleanup(); return fail(c, FSEQ_E_OOM, "restored founders output buffer"); }
	std::vector<uint64_t> seg(2 * S);
	for (size_t s = 0; s < S; ++s) { seg[s] = c->segments[s].lb; seg[S + s] = c->segments[s].rb; }
	bool ok = true;
	do {
		if (hipMemcpyAsync(d_perm, permutations, S * X * 4, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		if (hipMemcpyAsync(d_seg, seg.data(), 2 * S * 8, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		if (hipMemcpyAsync(d_lut, c->code_to_byte, 256, hipMemcpyHostToDevice, st) != hipSuccess) { ok = false; break; }
		for (size_t r0 = 0; r0 < X && ok; r0 += batch)
		{
			size_t const nr = std::min(batch, X - r0);
			uint64_t const total = (uint64_t) nr * line;
			uint32_t const rows_per_wg = 16;
			hipLaunchKernelGGL(k_identity_fill, dim3(grid_for((total + ID_T * 16u - 1u) / (ID_T * 16u))), dim3(ID_T), 0, st, c->idn.ref, n_src, total, d_out);
			hipLaunchKernelGGL(k_founders_restored, dim3((uint32_t) S, (uint32_t) ((nr + rows_per_wg - 1) / rows_per_wg)), dim3(256), 0, st, c->d_msa, c->ld, c->p.m, n_src, c->bsh,
			                   d_perm, (uint32_t) X, d_seg, d_seg + S, (uint32_t) r0, (uint32_t) nr, rows_per_wg, d_lut, c->idn.kept, d_out);
			if (hipMemcpyAsync(h_out, d_out, nr * line, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { ok = false; break; }
			ok = fwrite(h_out, 1, nr * line, f) == nr * line;
		}
	} while (false);
	if (ok && hipGetLastError() != hipSuccess) ok = false;
	fflush(f);
	cleanup();
	if (!ok) return fail(c, FSEQ_E_HIP, "writing the restored founders from the device failed");
	return FSEQ_OK;
}

} // extern "C"
