// fseq_api_input.hip -- the part of the C ABI (include/fseq.h) that takes the input rows in column chunks of bounded memory:
// fseq_input_begin, fseq_input_chunk_columns, fseq_input_scan, fseq_input_columns, fseq_input_end and fseq_set_rows_streamed,
// and -- the second half of this file -- the same input with the identity columns dropped on the way: fseq_input_scan_identity,
// fseq_input_reduce, fseq_input_kept_columns, fseq_input_columns_kept, fseq_input_end_kept and
// fseq_set_rows_streamed_without_identity_columns.
//
// fseq_set_rows (csrc/fseq_path_setup.hip, upload_rows_device_impl) stages the m x n raw bytes on the device beside the packed
// alignment; here the device holds the packed alignment and two staging halves.  Chunk i is copied into half i & 1 on the
// context's second stream while the kernel of chunk i - 1 reads the other half on the first; an event per half and direction
// orders them (copied: the kernel may read; used: the next copy may overwrite).  A call returns when its copies are done, not
// its kernel.  The kernels are in fseq_input.hpp.  A translation unit of its own: nothing here is allocated or launched unless
// its entry points are called.
#include "fseq_ctx.hpp"
#include "fseq_input.hpp"
#include "fseq_input_reduced.hpp"
#include "fseq_input_kept_range.hpp"
#include "fseq_identity.hpp"

using namespace fseq;

namespace {

constexpr uint64_t DEFAULT_STAGING = 256ull << 20;

int no_begin(fseq_ctx *c) { return fail(c, FSEQ_E_ARG, "chunked input: no fseq_input_begin on this context (or another input has taken its place)"); }
int sharded(fseq_ctx *c) { return fail(c, FSEQ_E_UNSUPPORTED, "chunked input: sharded context: the alphabet exchange of the ranks is not built for this path"); }

void drop_alignment(fseq_ctx *c)
{
	c->d_msa_own.release(c);
	c->d_msa = nullptr;
	c->have_input = false;
}

// what scan and columns ask of a chunk; `at`: the column the pass has reached.  rows == nullptr: the place and width alone
int check_chunk(fseq_ctx *c, char const *who, uint64_t at, uint64_t c0, uint64_t ncols, uint8_t const *const *rows)
{
	fseq_ctx::Input const &in = c->in;
	char what[256];
	if (c0 != at)
	{
		snprintf(what, sizeof(what), "%s: the chunk starts at column %llu but the pass has reached column %llu (chunks tile [0, n) in ascending order)", who,
		         (unsigned long long) c0, (unsigned long long) at);
		return fail(c, FSEQ_E_ARG, what);
	}
	if (0 == ncols || ncols > in.chunk_cols || ncols > c->p.n - c0)
	{
		snprintf(what, sizeof(what), "%s: a chunk of %llu columns at column %llu: at least 1, at most fseq_input_chunk_columns = %llu and within n = %llu", who,
		         (unsigned long long) ncols, (unsigned long long) c0, (unsigned long long) in.chunk_cols, (unsigned long long) c->p.n);
		return fail(c, FSEQ_E_ARG, what);
	}
	for (uint32_t r = 0; rows && r < c->p.m; ++r)
		if (!rows[r]) return fail(c, FSEQ_E_ARG, "null row pointer");
	return FSEQ_OK;
}

// the chunk's rows into the half of this call, on stream2; stream then waits for them.  *stage_out: the half, *rs_out: its row stride
int stage_chunk(fseq_ctx *c, uint64_t ncols, uint8_t const *const *rows, uint8_t **stage_out, size_t *rs_out, uint32_t *half_out)
{
	fseq_ctx::Input &in = c->in;
	uint32_t const h = (uint32_t) (in.calls & 1u), m = c->p.m;
	size_t const rs = ((size_t) ncols + 15) & ~size_t(15);
	uint8_t *const stage = in.stage.base + (size_t) h * in.half_bytes;
	if (in.calls >= 2) HIP_TRY(c, hipStreamWaitEvent(c->stream2, in.used[h], 0));
	// rows of one matrix (a constant, non-negative step between them) go up in one strided copy, others row by row
	ptrdiff_t const step = m > 1 ? rows[1] - rows[0] : 0;
	bool strided = m > 1 && step >= (ptrdiff_t) ncols;
	for (uint32_t r = 2; strided && r < m; ++r) strided = rows[r] - rows[r - 1] == step;
	if (strided)
		HIP_TRY(c, hipMemcpy2DAsync(stage, rs, rows[0], (size_t) step, (size_t) ncols, m, hipMemcpyHostToDevice, c->stream2));
	else
		for (uint32_t r = 0; r < m; ++r)
		{
			hipError_t const e = hipMemcpyAsync(stage + (size_t) r * rs, rows[r], (size_t) ncols, hipMemcpyHostToDevice, c->stream2);
			if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "chunked input: row copy", e);
		}
	HIP_TRY(c, hipEventRecord(in.copied[h], c->stream2));
	HIP_TRY(c, hipStreamWaitEvent(c->stream, in.copied[h], 0));
	*stage_out = stage; *rs_out = rs; *half_out = h;
	return FSEQ_OK;
}

// behind the kernel's launch: the half is free again when the kernel is done; the caller's bytes when the copies are
int finish_chunk(fseq_ctx *c, uint32_t h)
{
	fseq_ctx::Input &in = c->in;
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(in.used[h], c->stream));
	++in.calls;
	HIP_TRY(c, hipEventSynchronize(in.copied[h]));
	return FSEQ_OK;
}

// the first fseq_input_columns: the code table from the alphabet (dense codes in ascending byte order), the alignment
int fix_table(fseq_ctx *c)
{
	fseq_ctx::Input &in = c->in;
	if (!in.given)
	{
		HIP_TRY(c, hipMemcpyAsync(in.present, in.words, 32, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
	}
	uint8_t table[256];
	uint32_t sigma = 0;
	for (uint32_t b = 0; b < 256; ++b)
		if ((in.present[b >> 5] >> (b & 31u)) & 1u) ++sigma;
	if (0 == sigma) return fail(c, FSEQ_E_ARG, "chunked input: empty alphabet");
	uint32_t code = 0;
	for (uint32_t b = 0; b < 256; ++b)
		if ((in.present[b >> 5] >> (b & 31u)) & 1u) { table[b] = (uint8_t) code; c->code_to_byte[code] = (uint8_t) b; ++code; }
		else table[b] = 0xFF;
	c->sigma = sigma;
	c->bsh = sigma <= 4 ? 2u : sigma <= 16 ? 1u : 0u;              // (as alloc_msa, csrc/fseq_path_setup.hip)
	uint32_t const col_bytes = (uint32_t) (((uint64_t) c->p.m + (1u << c->bsh) - 1u) >> c->bsh);
	c->ld = ((size_t) col_bytes + 15) & ~size_t(15);
	drop_alignment(c);
	int const rc = c->d_msa_own.alloc(c, c->ld * (size_t) c->p.n + 16);
	if (rc) return rc;
	c->d_msa = c->d_msa_own.base;
	HIP_TRY(c, hipMemcpy(in.table, table, 256, hipMemcpyHostToDevice));
	in.table_ready = true;
	return FSEQ_OK;
}

int abandon(fseq_ctx *c, int rc)
{
	std::string const keep = c->err;
	(void) hipStreamSynchronize(c->stream2);
	(void) hipStreamSynchronize(c->stream);
	c->free_input();
	drop_alignment(c);
	c->err = keep;
	return rc;
}

// ---- the input with the identity columns dropped on the way ----

uint32_t grid_for(uint64_t groups, uint64_t most) { return (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(groups, most)); }

// a buffer of one context becomes another's, with its place in the accounts of both (fseq_debug_device_bytes)
template <typename T>
void hand_over(fseq_ctx *from, fseq_ctx *to, DevBuf<T> &src, DevBuf<T> &dst)
{
	dst.release(to);
	auto it = from->alloc_sizes.find(static_cast<void *>(src.base));
	size_t const bytes = it != from->alloc_sizes.end() ? it->second : 0;
	if (it != from->alloc_sizes.end()) { from->alloc_total -= bytes; from->alloc_sizes.erase(it); }
	to->alloc_sizes[static_cast<void *>(src.base)] = bytes;
	to->alloc_total += bytes;
	to->alloc_peak = std::max(to->alloc_peak, to->alloc_total);
	dst = src;
	src = DevBuf<T>{};
}

// the first fseq_input_scan_identity: the mask, the reference row and the accumulator of a chunk
int begin_identity_scan(fseq_ctx *c)
{
	fseq_ctx::Input &in = c->in;
	size_t const n = (size_t) c->p.n;
	size_t const words = input_identity_acc_words(std::min<uint64_t>(in.chunk_cols, c->p.n));
	int rc;
	if ((rc = in.id_mask.alloc(c, n)) || (rc = in.id_ref.alloc(c, n)) || (rc = in.id_acc.alloc(c, words)))
	{
		char what[320];
		snprintf(what, sizeof(what), "fseq_input_scan_identity: a mask and a reference row of %zu bytes each, %zu bytes of accumulators: %s", n, words * 4, c->err.c_str());
		release_all(c, in.id_mask, in.id_ref, in.id_acc);
		return fail(c, rc, what);
	}
	HIP_TRY(c, hipMemsetAsync(in.id_acc, 0, words * 4, c->stream));
	in.scan_mode = 2;
	return FSEQ_OK;
}

int bad_byte(fseq_ctx *c, uint32_t b)
{
	char what[160];
	snprintf(what, sizeof(what), "chunked input: the rows hold the byte 0x%02X (%u), which is not in the alphabet", b, b);
	return fail(c, FSEQ_E_ARG, what);
}

} // namespace

extern "C" {

int fseq_input_begin(fseq_ctx *c, uint8_t const *alphabet, uint32_t alphabet_size, uint64_t staging_bytes)
{
	if (!c) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	uint32_t present[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (alphabet)
	{
		if (0 == alphabet_size || alphabet_size > 256) return fail(c, FSEQ_E_ARG, "chunked input: an alphabet holds 1 to 256 byte values");
		for (uint32_t i = 0; i < alphabet_size; ++i)
		{
			uint32_t const b = alphabet[i];
			if ((present[b >> 5] >> (b & 31u)) & 1u)
			{
				char what[96];
				snprintf(what, sizeof(what), "chunked input: the alphabet lists the byte 0x%02X (%u) twice", b, b);
				return fail(c, FSEQ_E_ARG, what);
			}
			present[b >> 5] |= 1u << (b & 31u);
		}
	}
	uint64_t const staging = staging_bytes ? staging_bytes : DEFAULT_STAGING;
	uint64_t const half = (staging / 2) & ~15ull;
	// a chunk's rows are padded to 16 bytes in the half: whole 16-byte pieces of m rows
	uint64_t const chunk = std::min<uint64_t>((half / c->p.m) & ~15ull, 0x7FFFFFF0ull);
	if (chunk < 16)
	{
		char what[160];
		snprintf(what, sizeof(what), "chunked input: a staging of %llu bytes holds no column of %u rows: %llu bytes needed (two halves of 16 x m)",
		         (unsigned long long) staging, c->p.m, 32ull * c->p.m);
		return fail(c, FSEQ_E_ARG, what);
	}
	(void) hipSetDevice(c->p.device);
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	int rc;
	if ((rc = discard_input(c))) return rc;                        // (ends a chunked input under way, too)
	fseq_ctx::Input &in = c->in;
	in = fseq_ctx::Input{};
	if ((rc = in.stage.alloc(c, (size_t) (2 * half))) || (rc = in.words.alloc(c, 16)) || (rc = in.table.alloc(c, 256))) { c->free_input(); return rc; }
	for (int h = 0; h < 2; ++h)
		if (hipEventCreateWithFlags(&in.copied[h], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&in.used[h], hipEventDisableTiming) != hipSuccess)
		{ c->free_input(); return fail(c, FSEQ_E_HIP, "chunked input: event"); }
	hipError_t const e = hipMemsetAsync(in.words, 0, 64, c->stream);
	if (e != hipSuccess) { c->free_input(); return fail(c, FSEQ_E_HIP, "chunked input: memset", e); }
	in.given = alphabet != nullptr;
	memcpy(in.present, present, sizeof(present));
	in.half_bytes = half;
	in.chunk_cols = chunk;
	in.open = true;
	return FSEQ_OK;
}

uint64_t fseq_input_chunk_columns(fseq_ctx const *c) { return c && c->in.open ? c->in.chunk_cols : 0; }

int fseq_input_scan(fseq_ctx *c, uint64_t c0, uint64_t ncols, uint8_t const *const *rows)
{
	if (!c || !rows) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (in.given) return fail(c, FSEQ_E_ARG, "fseq_input_scan: the alphabet was supplied to fseq_input_begin");
	if (2 == in.scan_mode) return fail(c, FSEQ_E_ARG, "fseq_input_scan: this input is scanned by fseq_input_scan_identity (one scan entry per input)");
	if (in.table_ready) return fail(c, FSEQ_E_ARG, "fseq_input_scan: the code table is fixed: fseq_input_columns has begun");
	int rc = check_chunk(c, "fseq_input_scan", in.scanned, c0, ncols, rows);
	if (rc) return rc;
	in.scan_mode = 1;
	(void) hipSetDevice(c->p.device);
	uint8_t *stage; size_t rs; uint32_t h;
	if ((rc = stage_chunk(c, ncols, rows, &stage, &rs, &h))) return rc;
	uint64_t const pieces = (uint64_t) c->p.m * ((ncols + 15) / 16);
	uint32_t const grid = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((pieces + IN_T - 1) / IN_T, 4096));
	hipLaunchKernelGGL(k_input_presence, dim3(grid), dim3(IN_T), 0, c->stream, stage, rs, c->p.m, (uint32_t) ncols, in.words);
	if ((rc = finish_chunk(c, h))) return rc;
	in.scanned += ncols;
	return FSEQ_OK;
}

int fseq_input_columns(fseq_ctx *c, uint64_t c0, uint64_t ncols, uint8_t const *const *rows)
{
	if (!c || !rows) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_columns: fseq_input_reduce has made a context over the kept columns: its chunks go to fseq_input_columns_kept");
	if (!in.given && in.scanned != c->p.n)
	{
		char what[160];
		snprintf(what, sizeof(what), "fseq_input_columns: no alphabet yet: fseq_input_scan has covered %llu of %llu columns", (unsigned long long) in.scanned,
		         (unsigned long long) c->p.n);
		return fail(c, FSEQ_E_ARG, what);
	}
	int rc = check_chunk(c, "fseq_input_columns", in.encoded, c0, ncols, rows);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	if (!in.table_ready && (rc = fix_table(c))) return rc;
	uint32_t const row_tiles = (uint32_t) ((c->ld + IN_TILE_BYTES - 1) / IN_TILE_BYTES);
	uint64_t const tiles = ((ncols + IN_TILE_COLS - 1) / IN_TILE_COLS) * row_tiles;
	if (tiles > 0x7FFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "fseq_input_columns: more than 2^31 tiles in a chunk: use a smaller staging");
	uint8_t *stage; size_t rs; uint32_t h;
	if ((rc = stage_chunk(c, ncols, rows, &stage, &rs, &h))) return rc;
	uint32_t const check = c->sigma < 256 ? 1u : 0u;
	uint8_t *const dst = c->d_msa + (size_t) c0 * c->ld;
	uint32_t *const bad = in.words + 8;
#define FSEQ_INPUT_ENCODE(BSH) hipLaunchKernelGGL(k_input_encode<BSH>, dim3((uint32_t) tiles), dim3(IN_T), 0, c->stream, stage, rs, c->p.m, (uint32_t) ncols, \
	                                              in.table, check, dst, c->ld, row_tiles, bad)
	if (2 == c->bsh) FSEQ_INPUT_ENCODE(2);
	else if (1 == c->bsh) FSEQ_INPUT_ENCODE(1);
	else FSEQ_INPUT_ENCODE(0);
#undef FSEQ_INPUT_ENCODE
	if ((rc = finish_chunk(c, h))) return rc;
	in.encoded += ncols;
	return FSEQ_OK;
}

int fseq_input_end(fseq_ctx *c)
{
	if (!c) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_end: fseq_input_reduce has made a context over the kept columns: fseq_input_end_kept hands it out");
	if (in.encoded != c->p.n)
	{
		char what[160];
		snprintf(what, sizeof(what), "fseq_input_end: fseq_input_columns has covered %llu of %llu columns", (unsigned long long) in.encoded, (unsigned long long) c->p.n);
		return fail(c, FSEQ_E_ARG, what);
	}
	(void) hipSetDevice(c->p.device);
	uint32_t bad[8];
	hipError_t e = hipMemcpyAsync(bad, in.words + 8, 32, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { fail(c, FSEQ_E_HIP, "chunked input: the last chunks", e); return abandon(c, FSEQ_E_HIP); }
	c->free_input();
	for (uint32_t b = 0; b < 256; ++b)
		if ((bad[b >> 5] >> (b & 31u)) & 1u)
		{
			drop_alignment(c);
			char what[160];
			snprintf(what, sizeof(what), "chunked input: the rows hold the byte 0x%02X (%u), which is not in the alphabet", b, b);
			return fail(c, FSEQ_E_ARG, what);
		}
	forget_input_history(c);
	c->have_input = true;
	return FSEQ_OK;
}

int fseq_set_rows_streamed(fseq_ctx *c, uint8_t const *const *rows, uint64_t staging_bytes)
{
	if (!c || !rows) return FSEQ_E_ARG;
	for (uint32_t r = 0; r < c->p.m; ++r)
		if (!rows[r]) return fail(c, FSEQ_E_ARG, "null row pointer");
	int rc = fseq_input_begin(c, nullptr, 0, staging_bytes);
	if (rc) return rc;
	uint64_t width = c->in.chunk_cols;
	if ((width & ~63ull) >= 64) width &= ~63ull;
	std::vector<uint8_t const *> at(c->p.m);
	for (int pass = 0; pass < 2; ++pass)
		for (uint64_t c0 = 0; c0 < c->p.n; c0 += width)
		{
			uint64_t const ncols = std::min<uint64_t>(width, c->p.n - c0);
			for (uint32_t r = 0; r < c->p.m; ++r) at[r] = rows[r] + c0;
			rc = pass ? fseq_input_columns(c, c0, ncols, at.data()) : fseq_input_scan(c, c0, ncols, at.data());
			if (rc) return abandon(c, rc);
		}
	return fseq_input_end(c);
}

// ---- the same input with the identity columns dropped on the way: the scan pass finds them (k_input_identity), fseq_input_reduce
// makes the kept list and the context over the kept columns, the second pass packs only those (k_input_encode_kept).  The
// source's packed form never exists: src holds the staging, a mask and a reference row of n bytes each; the new context
// ld x kept bytes.  It belongs to src's input (in.half) until fseq_input_end_kept hands it out.

int fseq_input_scan_identity(fseq_ctx *c, uint64_t c0, uint64_t ncols, uint8_t const *const *rows)
{
	if (!c || !rows) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (1 == in.scan_mode) return fail(c, FSEQ_E_ARG, "fseq_input_scan_identity: this input is scanned by fseq_input_scan (one scan entry per input)");
	if (in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_scan_identity: fseq_input_reduce has been called: the scan is over");
	if (in.table_ready) return fail(c, FSEQ_E_ARG, "fseq_input_scan_identity: the code table is fixed: fseq_input_columns has begun");
	int rc = check_chunk(c, "fseq_input_scan_identity", in.scanned, c0, ncols, rows);
	if (rc) return rc;
	(void) hipSetDevice(c->p.device);
	if (2 != in.scan_mode && (rc = begin_identity_scan(c))) return rc;
	uint8_t *stage; size_t rs; uint32_t h;
	if ((rc = stage_chunk(c, ncols, rows, &stage, &rs, &h))) return rc;
	// pieces across, row slabs down: enough workgroups for the chip whatever the chunk's width, a slab a whole number of INR_RY rows
	uint32_t const m = c->p.m;
	uint32_t const gx = (uint32_t) (((ncols + 15) / 16 + INR_PX - 1) / INR_PX);
	uint32_t const slabs = grid_for(std::min<uint64_t>((1024 + gx - 1) / gx, ((uint64_t) m + INR_RY - 1) / INR_RY), 1024);
	uint32_t const slab_rows = (uint32_t) (((((uint64_t) m + slabs - 1) / slabs + INR_RY - 1) / INR_RY) * INR_RY);
	hipLaunchKernelGGL(k_input_identity, dim3(gx, slabs), dim3(IN_T), 0, c->stream, stage, rs, m, (uint32_t) ncols, slab_rows, in.words, in.id_acc);
	hipLaunchKernelGGL(k_input_identity_finish, dim3(grid_for(((ncols + 3) / 4 + IN_T - 1) / IN_T, 1024)), dim3(IN_T), 0, c->stream, stage, (uint32_t) ncols,
	                   in.id_acc, in.id_mask + c0, in.id_ref + c0);
	if ((rc = finish_chunk(c, h))) return rc;
	in.scanned += ncols;
	return FSEQ_OK;
}

int fseq_input_reduce(fseq_ctx *c, fseq_params const *params, fseq_identity_summary *summary)
{
	if (!c || !params) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: called twice on one input");
	if (2 != in.scan_mode || in.scanned != c->p.n)
	{
		char what[200];
		snprintf(what, sizeof(what), "fseq_input_reduce: the identity columns are not known yet: fseq_input_scan_identity has covered %llu of %llu columns",
		         (unsigned long long) (2 == in.scan_mode ? in.scanned : 0), (unsigned long long) c->p.n);
		return fail(c, FSEQ_E_ARG, what);
	}
	if (params->n != 0) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: params->n must be 0 (it becomes the number of kept columns)");
	if (params->m != 0 && params->m != c->p.m) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: params->m must be 0 or the source's");
	if (params->device != c->p.device) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: params->device must be the source's device");
	if (0 == params->segment_length) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: params->segment_length must be positive");
	uint64_t const n = c->p.n;
	if (n >= 0xFFFFFFFFull) return fail(c, FSEQ_E_ARG, "fseq_input_reduce: a source of 2^32 - 1 columns or more (the kept list holds 32-bit columns)");
	(void) hipSetDevice(c->p.device);
	hipStream_t const st = c->stream;

	// the alphabet of the WHOLE source: what the scans found, or the supplied one, which must hold what they found
	uint32_t found[8];
	HIP_TRY(c, hipMemcpyAsync(found, in.words, 32, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	if (in.given)
	{
		for (uint32_t b = 0; b < 256; ++b)
			if (((found[b >> 5] & ~in.present[b >> 5]) >> (b & 31u)) & 1u)
			{
				(void) hipStreamSynchronize(c->stream2);
				c->free_input();                                       // (as fseq_input_end: the context is left without an input)
				return bad_byte(c, b);
			}
	}
	else memcpy(in.present, found, sizeof(found));
	uint8_t table[256], code_to_byte[256] = {};
	uint32_t sigma = 0;
	for (uint32_t b = 0; b < 256; ++b)
		if ((in.present[b >> 5] >> (b & 31u)) & 1u) { table[b] = (uint8_t) sigma; code_to_byte[sigma] = (uint8_t) b; ++sigma; }
		else table[b] = 0xFF;
	if (0 == sigma) return fail(c, FSEQ_E_ARG, "chunked input: empty alphabet");
	uint32_t const bsh = sigma <= 4 ? 2u : sigma <= 16 ? 1u : 0u;      // (as fix_table)
	size_t const ld = ((size_t) (((uint64_t) c->p.m + (1u << bsh) - 1u) >> bsh) + 15) & ~size_t(15);

	// the kept list: the scan of fseq_identity.hpp on the finished mask
	uint32_t const ntiles = (uint32_t) ((n + ID_TILE - 1u) / ID_TILE);
	DevTemp<uint32_t> d_tiles(c);
	int rc;
	if ((rc = d_tiles.alloc((size_t) ntiles + 1))) return rc;
	hipEvent_t ev[2] = {nullptr, nullptr};
	struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 2; ++i) if (e[i]) (void) hipEventDestroy(e[i]); } } guard{ev};
	HIP_TRY(c, hipEventCreate(&ev[0]));
	HIP_TRY(c, hipEventCreate(&ev[1]));
	HIP_TRY(c, hipEventRecord(ev[0], st));
	hipLaunchKernelGGL(k_identity_count, dim3(ntiles), dim3(ID_T), 0, st, (uint8_t const *) in.id_mask, n, (uint32_t *) d_tiles);
	hipLaunchKernelGGL(k_identity_offsets, dim3(1), dim3(ID_T), 0, st, (uint32_t *) d_tiles, ntiles);
	HIP_TRY(c, hipGetLastError());
	uint32_t kept32 = 0;
	HIP_TRY(c, hipMemcpyAsync(&kept32, d_tiles + ntiles, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	uint64_t const kept = kept32;
	if (kept > n) return fail(c, FSEQ_E_HIP, "fseq_input_reduce: the scan of the mask counts more kept columns than there are columns");
	if (0 == kept)
	{
		// nothing of the identity pass stays: the input holds what fseq_input_begin allocated and the alphabet of the whole source,
		// so it may go on as an ordinary one (fseq_input_columns) or give way to a new fseq_input_begin
		release_all(c, in.id_mask, in.id_ref, in.id_acc);
		in.scan_mode = 1;
		return fail(c, FSEQ_E_ARG, "every column is an identity column: nothing is left to segment");
	}

	// the new context: an ordinary one over the kept columns, its alignment allocated at exactly their number
	fseq_params p = *params;
	p.m = c->p.m;
	p.n = kept;
	fseq_ctx *d = nullptr;
	if ((rc = fseq_create(&p, &d))) return fail(c, rc, "fseq_input_reduce: fseq_create of the new context failed");
	std::vector<uint32_t> kept_h;
	try { kept_h.resize((size_t) kept); }
	catch (std::bad_alloc const &) { fseq_destroy(d); return fail(c, FSEQ_E_OOM, "fseq_input_reduce: kept-column list (host)"); }
	if ((rc = d->d_msa_own.alloc(d, ld * (size_t) kept + 16)) || (rc = d->idn.kept.alloc(d, (size_t) kept)))
	{
		char what[400];
		snprintf(what, sizeof(what), "fseq_input_reduce: %llu kept columns of %zu bytes and %llu column indices (the mask and the reference row of %llu bytes each are held already): %s",
		         (unsigned long long) kept, ld, (unsigned long long) kept, (unsigned long long) n, d->err.c_str());
		fseq_destroy(d);
		return fail(c, rc, what);
	}
	auto give_up = [&](char const *what, hipError_t e) { (void) hipStreamSynchronize(st); fseq_destroy(d); return fail(c, FSEQ_E_HIP, what, e); };
	hipLaunchKernelGGL(k_identity_scatter, dim3(ntiles), dim3(ID_T), 0, st, (uint8_t const *) in.id_mask, n, (uint32_t const *) d_tiles, (uint32_t *) d->idn.kept);
	hipError_t e;
	if ((e = hipGetLastError()) != hipSuccess) return give_up("fseq_input_reduce: scatter launch", e);
	if ((e = hipEventRecord(ev[1], st)) != hipSuccess) return give_up("fseq_input_reduce: event", e);
	if ((e = hipMemcpyAsync(kept_h.data(), d->idn.kept, (size_t) kept * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return give_up("fseq_input_reduce: kept-column list", e);
	if ((e = hipMemcpyAsync(in.table, table, 256, hipMemcpyHostToDevice, st)) != hipSuccess) return give_up("fseq_input_reduce: code table", e);
	if ((e = hipStreamSynchronize(st)) != hipSuccess) return give_up("fseq_input_reduce: scatter", e);
	float ms = 0.f;
	(void) hipEventElapsedTime(&ms, ev[0], ev[1]);
	d->d_msa = d->d_msa_own.base;
	d->sigma = sigma;
	memcpy(d->code_to_byte, code_to_byte, sizeof(d->code_to_byte));
	d->bsh = bsh;
	d->ld = ld;
	d->idn.n_src = n;
	d->idn.identity = n - kept;
	hand_over(c, d, in.id_mask, d->idn.mask);
	hand_over(c, d, in.id_ref, d->idn.ref);
	in.id_acc.release(c);
	in.kept.swap(kept_h);
	in.half = d;
	in.reduced = true;
	in.table_ready = true;
	if (summary) *summary = fseq_identity_summary{n, n - kept, kept, (double) ms};
	return FSEQ_OK;
}

int fseq_input_kept_columns(fseq_ctx *c, uint64_t c0, uint64_t ncols, uint64_t *count)
{
	if (!c || !count) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input const &in = c->in;
	if (!in.open) return no_begin(c);
	if (!in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_kept_columns: no kept-column list yet: fseq_input_reduce has not been called");
	uint64_t k0 = 0, k1 = 0;
	if (char const *why = input_kept_range(in.kept.data(), (uint64_t) in.kept.size(), c0, ncols, &k0, &k1)) return fail(c, FSEQ_E_ARG, why);
	*count = k1 - k0;
	return FSEQ_OK;
}

int fseq_input_columns_kept(fseq_ctx *c, uint64_t c0, uint64_t ncols, uint8_t const *const *rows)
{
	if (!c) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (!in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_columns_kept: no kept-column list yet: fseq_input_reduce has not been called");
	int rc = check_chunk(c, "fseq_input_columns_kept", in.encoded, c0, ncols, nullptr);
	if (rc) return rc;
	uint64_t k0 = 0, k1 = 0;
	if (char const *why = input_kept_range(in.kept.data(), (uint64_t) in.kept.size(), c0, ncols, &k0, &k1)) return fail(c, FSEQ_E_ARG, why);
	if (k0 == k1) { in.encoded += ncols; return FSEQ_OK; }           // no kept column: no copy, no launch (rows may be NULL)
	if (!rows) return fail(c, FSEQ_E_ARG, "fseq_input_columns_kept: no rows for a chunk that holds kept columns");
	for (uint32_t r = 0; r < c->p.m; ++r)
		if (!rows[r]) return fail(c, FSEQ_E_ARG, "null row pointer");
	(void) hipSetDevice(c->p.device);
	fseq_ctx *const d = in.half;
	uint32_t const row_tiles = (uint32_t) ((d->ld + IN_TILE_BYTES - 1) / IN_TILE_BYTES);
	uint64_t const tiles = ((k1 - k0 + IN_TILE_COLS - 1) / IN_TILE_COLS) * row_tiles;
	if (tiles > 0x7FFFFFFFull) return fail(c, FSEQ_E_UNSUPPORTED, "fseq_input_columns_kept: more than 2^31 tiles in a chunk: use a smaller staging");
	uint8_t *stage; size_t rs; uint32_t h;
	if ((rc = stage_chunk(c, ncols, rows, &stage, &rs, &h))) return rc;
	uint32_t const check = d->sigma < 256 ? 1u : 0u;
	uint32_t *const bad = in.words + 8;
#define FSEQ_INPUT_ENCODE_KEPT(BSH) hipLaunchKernelGGL(k_input_encode_kept<BSH>, dim3((uint32_t) tiles), dim3(IN_T), 0, c->stream, stage, rs, c->p.m, c0, \
	                                                   (uint32_t const *) d->idn.kept, k0, k1, in.table, check, d->d_msa, d->ld, row_tiles, bad)
	if (2 == d->bsh) FSEQ_INPUT_ENCODE_KEPT(2);
	else if (1 == d->bsh) FSEQ_INPUT_ENCODE_KEPT(1);
	else FSEQ_INPUT_ENCODE_KEPT(0);
#undef FSEQ_INPUT_ENCODE_KEPT
	if ((rc = finish_chunk(c, h))) return rc;
	in.encoded += ncols;
	return FSEQ_OK;
}

int fseq_input_end_kept(fseq_ctx *c, fseq_ctx **out)
{
	if (!c || !out) return FSEQ_E_ARG;
	*out = nullptr;
	if (c->sh.on) return sharded(c);
	fseq_ctx::Input &in = c->in;
	if (!in.open) return no_begin(c);
	if (!in.reduced) return fail(c, FSEQ_E_ARG, "fseq_input_end_kept: no context over the kept columns: fseq_input_reduce has not been called");
	if (in.encoded != c->p.n)
	{
		char what[160];
		snprintf(what, sizeof(what), "fseq_input_end_kept: fseq_input_columns_kept has covered %llu of %llu columns", (unsigned long long) in.encoded, (unsigned long long) c->p.n);
		return fail(c, FSEQ_E_ARG, what);
	}
	(void) hipSetDevice(c->p.device);
	uint32_t bad[8];
	hipError_t e = hipMemcpyAsync(bad, in.words + 8, 32, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { fail(c, FSEQ_E_HIP, "chunked input: the last chunks", e); return abandon(c, FSEQ_E_HIP); }
	fseq_ctx *const d = in.half;
	in.half = nullptr;
	c->free_input();
	for (uint32_t b = 0; b < 256; ++b)
		if ((bad[b >> 5] >> (b & 31u)) & 1u)
		{
			fseq_destroy(d);
			return bad_byte(c, b);
		}
	d->idn.have = true;
	d->have_input = true;
	*out = d;
	return FSEQ_OK;
}

int fseq_set_rows_streamed_without_identity_columns(fseq_ctx *c, uint8_t const *const *rows, uint64_t staging_bytes, fseq_params const *params, fseq_ctx **out,
                                                    fseq_identity_summary *summary)
{
	if (!c || !rows || !params || !out) return FSEQ_E_ARG;
	*out = nullptr;
	for (uint32_t r = 0; r < c->p.m; ++r)
		if (!rows[r]) return fail(c, FSEQ_E_ARG, "null row pointer");
	int rc = fseq_input_begin(c, nullptr, 0, staging_bytes);
	if (rc) return rc;
	uint64_t width = c->in.chunk_cols;
	if ((width & ~63ull) >= 64) width &= ~63ull;
	std::vector<uint8_t const *> at(c->p.m);
	for (int pass = 0; pass < 2; ++pass)
	{
		for (uint64_t c0 = 0; c0 < c->p.n; c0 += width)
		{
			uint64_t const ncols = std::min<uint64_t>(width, c->p.n - c0);
			for (uint32_t r = 0; r < c->p.m; ++r) at[r] = rows[r] + c0;
			rc = pass ? fseq_input_columns_kept(c, c0, ncols, at.data()) : fseq_input_scan_identity(c, c0, ncols, at.data());
			if (rc) return abandon(c, rc);
		}
		if (!pass && (rc = fseq_input_reduce(c, params, summary))) return c->in.open ? abandon(c, rc) : rc;
	}
	return fseq_input_end_kept(c, out);
}

// fseq_debug_input_kept_range: input_kept_range on a caller-supplied kept list.  No device, no context.
int fseq_debug_input_kept_range(uint64_t const *kept, uint64_t n_kept, uint64_t c0, uint64_t ncols, uint64_t *k0, uint64_t *k1)
{
	if (!k0 || !k1) return FSEQ_E_ARG;
	return input_kept_range(kept, n_kept, c0, ncols, k0, k1) ? FSEQ_E_ARG : FSEQ_OK;
}

int fseq_debug_packed_columns(fseq_ctx *c, uint64_t c0, uint64_t c1, uint8_t *out, uint64_t *ld, uint32_t *bits)
{
	if (!c || !ld || !bits) return FSEQ_E_ARG;
	if (c->sh.on) return sharded(c);
	if (!c->have_input || !c->d_msa || c0 > c1 || c1 > c->p.n) return fail(c, FSEQ_E_ARG, "packed columns: no alignment resident, or columns out of range");
	*ld = c->ld;
	*bits = 8u >> c->bsh;
	if (!out || c0 == c1) return FSEQ_OK;
	(void) hipSetDevice(c->p.device);
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(out, c->d_msa + (size_t) c0 * c->ld, (size_t) (c1 - c0) * c->ld, hipMemcpyDeviceToHost));
	return FSEQ_OK;
}

} // extern "C"
