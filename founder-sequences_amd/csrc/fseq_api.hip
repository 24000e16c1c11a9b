// fseq_api.hip -- C ABI (include/fseq.h): the entry points of the segmentation path.
//
// Host side of what segmentation_lp_context drives through libdispatch queues
// (founder-sequences/segmentation_lp_context.cc:26-390): here one HIP stream, kernels per phase,
// and only the O(S) pieces (traceback walk lp.cc:191-224, segment merge lp.cc:335-390) on the CPU.
// There is deliberately NO CPU fallback for the column work: if the device or a kernel shape is
// unavailable the call fails with an error code.
// The context and the helpers every translation unit shares are in fseq_ctx.hpp.  The orchestration behind these entry points
// is in the path's units (fseq_path.hpp lists them: csrc/fseq_path_setup.hip, _dp, _pass1, _reduced, _attempt, _pass2), the debug entry points
// and the row-sharded sweep in csrc/fseq_api_debug.hip; the host joiners, their device front and the output writers are
// csrc/fseq_api_join.hip, the matcher csrc/fseq_api_match.hip, the identity columns csrc/fseq_api_identity.hip, the rows held out of the
// resident alignment csrc/fseq_api_rowsplit.hip and the chunked input csrc/fseq_api_input.hip.
#include "fseq_path.hpp"
#include "fseq_kernels.hpp"

#include <cassert>

using namespace fseq;

// What a run leaves behind for the next run in the same geometry: the result, the kernel choice, what phase A gave up, the plan of
// the representatives.  A tuning knob forgets this much (the input is the same one) ...
void fseq::forget_run_history(fseq_ctx *c)
{
	c->have_result = false;
	c->scan_lists = false;
	c->kernels_ready = false;
	c->bk_given_up = -1; c->bt_given_up = -1; c->red.memory.forget_input();
}

// ... and an input what was learnt of the input besides
void fseq::forget_input_history(fseq_ctx *c)
{
	forget_run_history(c);
	c->X_hint = 0;
	c->colmask_ready = false; c->shard_dp_full_sticky = false;
	c->bip_path = -1;
	c->rand_path = -1;
	c->score_path = -1;
}

// A new input takes this context: every input setter calls this once its arguments are in order and before it touches the
// alignment.  The work buffers go, and with them everything ensure_work_buffers decides only where it allocates (the form and
// packing of the stride states, their spacing, the workspace's rebase, the buffers sized by the block count): the next run
// lays them out for the new alphabet and packing.  The result and the last match go too.  A context made by
// fseq_create_without_identity_columns holds the relation of its columns to its source's: it refuses another input.
int fseq::take_new_input(fseq_ctx *c)
{
	if (c->idn.have)
		return fail(c, FSEQ_E_ARG, "a context made by fseq_create_without_identity_columns takes no other input (its identity relation belongs to the columns it was made from)");
	if (c->hold.have)
		return fail(c, FSEQ_E_ARG, "a context made by fseq_create_without_rows takes no other input (its held-out rows belong to the alignment it was made from)");
	(void) hipSetDevice(c->p.device);
	if (c->stream) (void) hipStreamSynchronize(c->stream);
	free_work(c);
	c->free_match();
	forget_input_history(c);
	return FSEQ_OK;
}

// the chunked input's begin (csrc/fseq_api_input.hip): the alignment goes as well, before the staging is allocated
int fseq::discard_input(fseq_ctx *c)
{
	int const rc = take_new_input(c);
	if (rc) return rc;
	free_msa(c);
	return FSEQ_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" {

uint32_t fseq_abi_version(void) { return FSEQ_ABI_VERSION; }

char const *fseq_strerror(int code)
{
	switch (code)
	{
		case FSEQ_OK: return "ok";
		case FSEQ_E_ARG: return "bad argument";
		case FSEQ_E_NO_REDUCTION: return "unable to reduce the number of sequences";
		case FSEQ_E_HIP: return "HIP runtime error";
		case FSEQ_E_OOM: return "out of device memory";
		case FSEQ_E_UNSUPPORTED: return "unsupported shape for this build";
		case FSEQ_E_PEER: return "another rank of the sharded run failed";
		default: return "unknown";
	}
}

int fseq_create(fseq_params const *params, fseq_ctx **out)
{
	if (!params || !out) return FSEQ_E_ARG;
	*out = nullptr;
	if (0 == params->m || 0 == params->n || 0 == params->segment_length) return FSEQ_E_ARG;
	if (params->n >= 0xFFFFFFF0ull) return FSEQ_E_ARG;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FSEQ_E_HIP;
	if (params->device < 0 || params->device >= ndev) return FSEQ_E_ARG;
	if (hipSetDevice(params->device) != hipSuccess) return FSEQ_E_HIP;
	fseq_ctx *c = new fseq_ctx();
	c->p = *params;
	c->tune.from_environment();                  // the only look at the environment: fseq_debug_set_tuning changes a knob afterwards
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { fseq_destroy(c); return FSEQ_E_HIP; }
	if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) { fseq_destroy(c); return FSEQ_E_HIP; }
	if (hipEventCreateWithFlags(&c->ev.dp_reset, hipEventDisableTiming) != hipSuccess) { fseq_destroy(c); return FSEQ_E_HIP; }
	for (hipEvent_t *e : c->ev.timed())
		if (hipEventCreate(e) != hipSuccess) { fseq_destroy(c); return FSEQ_E_HIP; }
	*out = c;
	return FSEQ_OK;
}

void fseq_destroy(fseq_ctx *c)
{
	if (!c) return;
	(void) hipSetDevice(c->p.device);
	if (c->stream) (void) hipStreamSynchronize(c->stream);
	free_msa(c);
	free_work(c);
	c->free_match();
	c->free_identity();
	c->free_held_out();
	c->free_input();
	assert(c->alloc_sizes.empty() && c->alloc_total == 0);       // (a buffer free_work does not know of)
	for (hipEvent_t *e : c->ev.timed()) if (*e) (void) hipEventDestroy(*e);
	if (c->ev.dp_reset) (void) hipEventDestroy(c->ev.dp_reset);
	for (auto &e : c->lw.ev) if (e) (void) hipEventDestroy(e);
	if (c->h_pin) (void) hipHostFree(c->h_pin);
	if (c->h_red_pin) (void) hipHostFree(c->h_red_pin);
	if (c->h_red_pin2) (void) hipHostFree(c->h_red_pin2);
	for (auto &s_ : c->red_st) if (s_) (void) hipStreamDestroy(s_);
	for (hipEvent_t *e_ : c->red_ev.all()) if (*e_) (void) hipEventDestroy(*e_);
	if (c->stream2) (void) hipStreamDestroy(c->stream2);
	if (c->stream) (void) hipStreamDestroy(c->stream);
	delete c;
}

char const *fseq_last_error(fseq_ctx const *c) { return c ? c->err.c_str() : "null context"; }

int fseq_set_matrix(fseq_ctx *c, uint8_t const *base, size_t row_stride, size_t col_stride)
{
	if (!c || !base) return FSEQ_E_ARG;
	if (int const rc = take_new_input(c)) return rc;
	if (1 == col_stride)
	{
		// row-major view: the same device path as fseq_set_rows
		std::vector<uint8_t const *> rows(c->p.m);
		for (uint32_t r = 0; r < c->p.m; ++r) rows[r] = base + (size_t) r * row_stride;
		return upload_rows_device(c, rows.data());
	}
	return set_alphabet_and_upload(c, base, row_stride, col_stride);     // any other layout: host encode + transpose
}

int fseq_set_rows(fseq_ctx *c, uint8_t const *const *rows)
{
	if (!c || !rows) return FSEQ_E_ARG;
	(void) hipSetDevice(c->p.device);
	for (uint32_t r = 0; r < c->p.m; ++r)
		if (!rows[r]) return fail(c, FSEQ_E_ARG, "null row pointer");
	if (int const rc = take_new_input(c)) return rc;
	return upload_rows_device(c, rows);
}

// borrowed columns: every code must be < sigma (the owned upload paths build the code table themselves)
static int check_borrowed_codes(fseq_ctx *c)
{
	if (c->sigma >= (1u << (8u >> c->bsh))) return FSEQ_OK;          // every code the width can hold is allowed
	uint64_t const ncols = held_hi(c) - held_lo(c);
	if (!ncols) return FSEQ_OK;
	DevTemp<uint32_t> d_mx(c);
	int rc = d_mx.alloc(1);
	if (rc) return rc;
	uint32_t mx = 0;
	uint32_t const col_bytes = sym_bytes(c->p.m, c->bsh), tail = c->p.m & ((1u << c->bsh) - 1u);
	hipError_t e = hipMemsetAsync(d_mx, 0, 4, c->stream);
	if (e == hipSuccess)
	{
		hipLaunchKernelGGL(k_max_code, dim3((uint32_t) std::min<uint64_t>(ncols, 4096)), dim3(256), 0, c->stream,
		                   c->d_msa + held_lo(c) * c->ld, c->ld, col_bytes, ncols, c->bsh, tail, d_mx);
		e = hipMemcpyAsync(&mx, d_mx, 4, hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "checking the borrowed columns", e);
	if (mx >= c->sigma)
	{
		c->have_input = false;
		char what[128];
		snprintf(what, sizeof(what), "borrowed device columns hold the code %u but sigma is %u", mx, c->sigma);
		return fail(c, FSEQ_E_ARG, what);
	}
	return FSEQ_OK;
}

int fseq_set_device_columns(fseq_ctx *c, void const *d_codes, size_t ld, uint32_t sigma)
{
	if (!c || !d_codes) return FSEQ_E_ARG;
	if (ld < c->p.m || (ld & 15) || (reinterpret_cast<uintptr_t>(d_codes) & 15))
		return fail(c, FSEQ_E_ARG, "device columns: ld must be >= m and a multiple of 16, base 16-byte aligned");
	if (sigma == 0 || sigma > 256) return fail(c, FSEQ_E_ARG, "sigma out of range");
	if (int const rc = take_new_input(c)) return rc;
	free_msa(c);
	c->d_msa = const_cast<uint8_t *>(static_cast<uint8_t const *>(d_codes)) - held_lo(c) * ld;
	c->ld = ld;
	c->bsh = 0;                              // borrowed columns are one code per byte
	c->sigma = sigma;
	for (uint32_t i = 0; i < 256; ++i) c->code_to_byte[i] = (uint8_t) i;
	c->have_input = true;
	return check_borrowed_codes(c);
}

int fseq_set_device_columns_packed(fseq_ctx *c, void const *d_packed, size_t ld_bytes, uint32_t sigma, uint32_t bits)
{
	if (!c || !d_packed) return FSEQ_E_ARG;
	if (bits != 2 && bits != 4 && bits != 8) return fail(c, FSEQ_E_ARG, "packed device columns: bits must be 2, 4 or 8");
	uint32_t const bsh = bits == 2 ? 2u : bits == 4 ? 1u : 0u;
	if (sigma == 0 || sigma > (1u << bits)) return fail(c, FSEQ_E_ARG, "sigma does not fit the code width");
	if (ld_bytes < sym_bytes(c->p.m, bsh) || (ld_bytes & 15) || (reinterpret_cast<uintptr_t>(d_packed) & 15))
		return fail(c, FSEQ_E_ARG, "packed device columns: ld_bytes must cover a column and be a multiple of 16, base 16-byte aligned");
	if (int const rc = take_new_input(c)) return rc;
	free_msa(c);
	c->d_msa = const_cast<uint8_t *>(static_cast<uint8_t const *>(d_packed)) - held_lo(c) * ld_bytes;
	c->ld = ld_bytes;
	c->bsh = bsh;
	c->sigma = sigma;
	for (uint32_t i = 0; i < 256; ++i) c->code_to_byte[i] = (uint8_t) i;
	c->have_input = true;
	return check_borrowed_codes(c);
}

uint64_t fseq_shard_xbuf_words(fseq_ctx const *c, uint32_t world)
{
	if (!c || 0 == world) return 0;
	// the largest exchanges: a whole DP array (keys, then lb, then size, one at a time), the hyper key blocks of
	// phase B (world x (2m + 1) words), the merge thresholds (2 words per traceback boundary <= n / L + 1)
	uint64_t const dp = c->p.n >= c->p.segment_length ? c->p.n - c->p.segment_length + 1 : 1;
	uint64_t const keys = (uint64_t) world * (2ull * c->p.m + 1);
	uint64_t const tb = 4 * (c->p.n / std::max<uint64_t>(1, c->p.segment_length) + 2) + 2;     // the gathered traceback entries (16 bytes each)
	return std::max<uint64_t>(std::max(std::max(dp, tb), keys), 1024) + 64;
}

int fseq_set_shard(fseq_ctx *c, uint32_t rank, uint32_t world, void *xbuf_device, uint64_t xbuf_words, fseq_allreduce_fn fn, void *user)
{
	if (!c || 0 == world || rank >= world) return FSEQ_E_ARG;
	if (c->have_input) return fail(c, FSEQ_E_ARG, "fseq_set_shard must be called before the input is set");
	if (1 == world) { c->sh = Shard{}; return FSEQ_OK; }
	if (c->lw.budget) return fail(c, FSEQ_E_UNSUPPORTED, "a list memory budget (fseq_set_list_memory) holds one GPU's lists in windows: not for sharded runs");
	if (!xbuf_device || !fn) return fail(c, FSEQ_E_ARG, "sharded run: exchange buffer and all-reduce function needed");
	if (c->p.n < 2 * c->p.segment_length) return fail(c, FSEQ_E_UNSUPPORTED, "the short path (n < 2L) is one sweep and does not shard");
	Shard sh;
	sh.on = true; sh.rank = rank; sh.world = world;
	sh.xbuf = static_cast<uint32_t *>(xbuf_device); sh.xwords = xbuf_words; sh.fn = fn; sh.user = user;
	c->sh = sh;
	block_geometry(c);
	uint64_t const need = fseq_shard_xbuf_words(c, world);
	if (xbuf_words < need) { c->sh = Shard{}; return fail(c, FSEQ_E_ARG, "exchange buffer too small (fseq_shard_xbuf_words)"); }
	bool const ok = shard_dp_plan_ok(c);
	if (!ok) { c->sh = Shard{}; return fail(c, FSEQ_E_UNSUPPORTED, "too few columns per rank for this segment length: use fewer ranks"); }
	return FSEQ_OK;
}

int fseq_shard_abort(fseq_ctx *c, int code)
{
	if (!c) return FSEQ_E_ARG;
	if (!c->sh.on) return FSEQ_OK;
	(void) hipSetDevice(c->p.device);
	shard_post_failure(c, code ? code : FSEQ_E_HIP);
	return FSEQ_OK;
}

int fseq_shard_columns(fseq_ctx const *c, uint64_t *first, uint64_t *last)
{
	if (!c || !first || !last) return FSEQ_E_ARG;
	*first = held_lo(c); *last = held_hi(c);
	return FSEQ_OK;
}

int fseq_shard_owner(fseq_ctx const *c, uint64_t rb, uint32_t *rank)
{
	if (!c || !rank || rb > c->p.n) return FSEQ_E_ARG;
	*rank = c->sh.on ? (uint32_t) std::min<uint64_t>(rb / ((uint64_t) c->sh.bpr * c->B), c->sh.active - 1u) : 0u;
	return FSEQ_OK;
}

int fseq_generate_synthetic(fseq_ctx *c, fseq_synth_spec const *spec)
{
	if (!c || !spec || 0 == spec->n_founders || 0 == spec->block_len || spec->kind > 1) return FSEQ_E_ARG;
	if (int const rc0 = take_new_input(c)) { shard_post_failure(c, rc0); return rc0; }
	char const *alpha = spec->kind ? "ACGTRYSWKMBDHVN-" : "ACGT";
	uint32_t const sigma = spec->kind ? 16u : 4u;
	c->sigma = sigma;
	int rc = alloc_msa(c);
	if (rc) { shard_post_failure(c, rc); return rc; }
	SynthArgs A;
	A.seed = spec->seed; A.n_founders = spec->n_founders; A.block_len = spec->block_len;
	A.mut_threshold = spec->mut_threshold; A.kind = spec->kind; A.sigma = sigma;
	for (uint32_t i = 0; i < 16; ++i) A.code_of_sym[i] = 0;
	for (uint32_t i = 0; i < sigma; ++i)
	{
		uint32_t rank = 0;
		for (uint32_t j = 0; j < sigma; ++j) rank += ((uint8_t) alpha[j] < (uint8_t) alpha[i]) ? 1u : 0u;
		A.code_of_sym[i] = (uint8_t) rank;
		c->code_to_byte[rank] = (uint8_t) alpha[i];
	}
	uint64_t const k_lo = held_lo(c), k_hi = held_hi(c);     // sharded: this rank's columns only
	if (k_hi > k_lo)
	{
		dim3 const grid((uint32_t) ((c->ld / 4 + 255) / 256), (uint32_t) std::min<uint64_t>(k_hi - k_lo, 65535));
		hipLaunchKernelGGL(k_synth, grid, dim3(256), 0, c->stream, A, c->d_msa, c->ld, c->p.m, k_lo, k_hi, c->bsh);
	}
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->have_input = true;
	return FSEQ_OK;
}

int fseq_get_matrix(fseq_ctx *c, uint64_t c0, uint64_t c1, uint8_t *out, size_t row_stride, size_t col_stride)
{
	if (!c || !out || !c->have_input || c0 > c1 || c1 > c->p.n) return FSEQ_E_ARG;
	if (c0 < held_lo(c) || c1 > held_hi(c)) return fail(c, FSEQ_E_ARG, "columns not held by this rank");
	(void) hipSetDevice(c->p.device);
	std::vector<uint8_t> buf((c1 - c0) * c->ld);
	uint32_t const bsh = c->bsh, smask = (1u << bsh) - 1u, bits = 8u >> bsh, cmask = (1u << bits) - 1u;
	HIP_TRY(c, hipMemcpy(buf.data(), c->d_msa + c0 * c->ld, buf.size(), hipMemcpyDeviceToHost));
	for (uint64_t col = c0; col < c1; ++col)
		for (uint32_t r = 0; r < c->p.m; ++r)
			out[(size_t) r * row_stride + (col - c0) * col_stride] =
				c->code_to_byte[(buf[(col - c0) * c->ld + (r >> bsh)] >> ((r & smask) * bits)) & cmask];
	return FSEQ_OK;
}

int fseq_run_segmentation(fseq_ctx *c, fseq_result *res)
{
	if (!c || !res) return FSEQ_E_ARG;
	if (!c->have_input) return fail(c, FSEQ_E_ARG, "no input set");
	(void) hipSetDevice(c->p.device);
	c->have_result = false;
	c->scan_lists = false;
	c->sh.closed = false;
	c->lw.on = false; c->lw.merge_windows = 0;
	if (!c->kernels_ready)
	{
		int rc = prepare_geometry(c);
		if (rc) { shard_post_failure(c, rc); return rc; }
	}
	// generate_context::calculate_segmentation, generate_context.cc:386-389
	if (c->p.n < 2 * c->p.segment_length)
	{
		if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "the short path (n < 2L) is one sweep and does not shard");
		return run_short_path(c, res);
	}
	int const rc = run_long_path(c, res);
	shard_post_failure(c, rc);                   // sharded: the other ranks learn of it in their next exchange
	return rc;
}

int fseq_set_progress(fseq_ctx *c, fseq_progress_fn fn, void *user)
{
	if (!c) return FSEQ_E_ARG;
	c->progress_fn = fn; c->progress_user = user;
	return FSEQ_OK;
}
uint64_t fseq_step_max(fseq_ctx const *c) { return c ? c->step_max.load(std::memory_order_relaxed) : 0; }
uint64_t fseq_current_step(fseq_ctx const *c) { return c ? c->current_step.load(std::memory_order_relaxed) : 0; }


/* replaces: nothing in the reference (one process, one address space).  A context that shares its device with other
 * contexts or ranks plans its pass-2 stride states inside `bytes` of device memory in all (0 = whatever is free). */
int fseq_set_memory_budget(fseq_ctx *c, uint64_t bytes)
{
	if (!c) return FSEQ_E_ARG;
	c->mem_budget = bytes;
	return FSEQ_OK;
}

int fseq_set_list_memory(fseq_ctx *c, uint64_t bytes)
{
	if (!c) return FSEQ_E_ARG;
	if (c->sh.on) return fail(c, FSEQ_E_UNSUPPORTED, "a list memory budget holds one GPU's lists in windows: not for sharded contexts");
	c->lw.budget = bytes;
	return FSEQ_OK;
}

int fseq_run_segmentation_batch(fseq_ctx *const *ctxs, size_t count, fseq_result *results, int *return_codes)
{
	if ((count && (!ctxs || !results || !return_codes))) return FSEQ_E_ARG;
	for (size_t i = 0; i < count; ++i)
		for (size_t j = 0; j < i; ++j)
			if (ctxs[i] == ctxs[j]) return FSEQ_E_ARG;                 // a context runs one alignment at a time
	std::vector<std::thread> workers;
	workers.reserve(count);
	for (size_t i = 1; i < count; ++i)
		workers.emplace_back([=]() { return_codes[i] = fseq_run_segmentation(ctxs[i], &results[i]); });
	if (count) return_codes[0] = fseq_run_segmentation(ctxs[0], &results[0]);
	for (auto &w : workers) w.join();
	return FSEQ_OK;
}

int fseq_get_traceback(fseq_ctx *c, fseq_dp_arg *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (int const rc = need_result(c, false)) return rc;
	std::copy(c->traceback.begin(), c->traceback.end(), out);
	return FSEQ_OK;
}

int fseq_get_segments(fseq_ctx *c, fseq_segment *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	if (int const rc = need_result(c, false)) return rc;
	std::copy(c->segments.begin(), c->segments.end(), out);
	return FSEQ_OK;
}

int fseq_boundary_state(fseq_ctx *c, uint64_t i, uint32_t *a_out, uint32_t *d_out)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c, false)) return rc;
	if (i >= c->segments.size()) return FSEQ_E_ARG;
	(void) hipSetDevice(c->p.device);
	size_t const m = c->p.m;
	if (i >= c->snap_slot.size() || c->snap_slot[i] < 0) return fail(c, FSEQ_E_ARG, "boundary state held by another rank (fseq_shard_owner)");
	size_t const slot = (size_t) c->snap_slot[i];
	if (a_out) HIP_TRY(c, hipMemcpy(a_out, c->d_snap_a + slot * m, m * 4, hipMemcpyDeviceToHost));
	if (d_out) HIP_TRY(c, hipMemcpy(d_out, c->d_snap_d + slot * m, m * 4, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

int fseq_short_path_runs(fseq_ctx *c, uint32_t *first_idx, uint32_t *run_len)
{
	if (!c) return FSEQ_E_ARG;
	if (int const rc = need_result(c, false)) return rc;
	if (!c->res.short_path) return FSEQ_E_ARG;
	if (first_idx) std::copy(c->sp_first.begin(), c->sp_first.end(), first_idx);
	if (run_len) std::copy(c->sp_len.begin(), c->sp_len.end(), run_len);
	return FSEQ_OK;
}

int fseq_get_timings(fseq_ctx const *c, fseq_timings *out)
{
	if (!c || !out) return FSEQ_E_ARG;
	*out = c->tm;
	return FSEQ_OK;
}

} // extern "C"
