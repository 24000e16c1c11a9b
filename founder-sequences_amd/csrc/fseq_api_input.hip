// fseq_api_input.hip -- the part of the C ABI (include/fseq.h) that takes the input rows in column chunks of bounded memory:
// fseq_input_begin, fseq_input_chunk_columns, fseq_input_scan, fseq_input_columns, fseq_input_end and fseq_set_rows_streamed.
//
// fseq_set_rows (csrc/fseq_path_setup.hip, upload_rows_device_impl) stages the m x n raw bytes on the device beside the packed
// alignment; here the device holds the packed alignment and two staging halves.  Chunk i is copied into half i & 1 on the
// context's second stream while the kernel of chunk i - 1 reads the other half on the first; an event per half and direction
// orders them (copied: the kernel may read; used: the next copy may overwrite).  A call returns when its copies are done, not
// its kernel.  The kernels are in fseq_input.hpp.  A translation unit of its own: nothing here is allocated or launched unless
// its entry points are called.
#include "fseq_ctx.hpp"
#include "fseq_input.hpp"

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

// what scan and columns ask of a chunk; `at`: the column the pass has reached
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
	for (uint32_t r = 0; r < c->p.m; ++r)
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
	if (in.table_ready) return fail(c, FSEQ_E_ARG, "fseq_input_scan: the code table is fixed: fseq_input_columns has begun");
	int rc = check_chunk(c, "fseq_input_scan", in.scanned, c0, ncols, rows);
	if (rc) return rc;
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
