// fseq_localpass.hpp -- the local pass of a partition step (fseq_core.hpp) over a thread's own rows, with the four running
// maxima as 16-bit halves of two registers.  For four symbols and values below 2^16 (phase C's value ids, KS = 16).
//
// The plain pass keeps run[0 .. 3] in a register each and pays, per row and symbol, a maximum, a compare and two selects:
// sixteen vector instructions a row, every one in the 4.2-cycle class (profiles/r03_valu_rates.txt).  Here
//   {run[1], run[0]} and {run[3], run[2]} are one register each and one v_pk_max_u16 raises two of them (the row's value
//     goes in through the instruction's operand select, no duplicate is made);
//   the row's own value is one byte select (v_perm_b32) out of the pair, its selector one multiply-add of the symbol;
//   the reset of the row's own symbol is an AND with two masks, each one byte select out of a constant: the selector's four
//     bytes are {3, 3, 2, 2} + symbol, a window that slides over eight constant bytes of which one is zero.  For the
//     symbols 0 .. 4 every selector byte is 2 .. 7, a byte of the constant: an unused position (symbol 4) resets nothing
//     by construction, without a compare and without a shift by the symbol.
// Eleven instructions a row, three of them (an add, two ANDs) in the 2.3-cycle class.
//
// The same text runs on the host (the two instructions restated in plain C++), where tests/test_local_pass_packed.py
// checks it against the plain pass, bit 15 of the values included: a signed packed maximum passes every end-to-end test.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSEQ_LP_HD __host__ __device__ __forceinline__
#else
#define FSEQ_LP_HD inline
#endif

namespace fseq {

// v_perm_b32: byte i of the result is chosen by byte i of sel out of the eight bytes {hi, lo} (0 .. 3: lo, 4 .. 7: hi);
// 8 .. 11 spread the sign of byte 1, 3, 5, 7; 12 is 0x00; anything above is 0xFF
FSEQ_LP_HD uint32_t lp_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_perm(hi, lo, sel);
#else
	uint64_t const src = ((uint64_t) hi << 32) | lo;
	uint8_t tab[16];
	for (int b = 0; b < 8; ++b) tab[b] = (uint8_t) (src >> (8 * b));
	for (int b = 8; b < 12; ++b) tab[b] = ((src >> (16 * (b - 8) + 15)) & 1u) ? 0xFFu : 0u;
	tab[12] = 0u; tab[13] = tab[14] = tab[15] = 0xFFu;
	uint32_t r = 0;
	for (int i = 0; i < 4; ++i)
	{
		uint32_t const b = (sel >> (8 * i)) & 0xFFu;
		r |= (uint32_t) (b < 16u ? tab[b] : 0xFFu) << (8 * i);
	}
	return r;
#endif
}

// v_pk_max_u16 of the two halves of p with v in BOTH halves (v < 2^16), unsigned
FSEQ_LP_HD uint32_t lp_pk_max_u16(uint32_t p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	typedef unsigned short lp_u16x2 __attribute__((ext_vector_type(2)));
	lp_u16x2 const a = __builtin_bit_cast(lp_u16x2, p);
	lp_u16x2 const b = {(unsigned short) v, (unsigned short) v};
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(a, b));
#else
	uint32_t const lo = p & 0xFFFFu, hi = p >> 16, w = v & 0xFFFFu;
	return (lo > w ? lo : w) | ((hi > w ? hi : w) << 16);
#endif
}

// the four running maxima: p01 = run[1] << 16 | run[0], p23 = run[3] << 16 | run[2]
struct PackedRuns { uint32_t p01 = 0, p23 = 0; };

// One row: value de < 2^16, symbol c in 0 .. 4 (4: an unused position, whose de is 0).  Returns the row's new value --
// max(run[c], de), 0 for c == 4 -- and leaves run[x] = max(run[x], de) for x != c, run[c] = 0.
FSEQ_LP_HD uint32_t local_pass_packed_row(PackedRuns &r, uint32_t de, uint32_t c)
{
	r.p01 = lp_pk_max_u16(r.p01, de);
	r.p23 = lp_pk_max_u16(r.p23, de);
	// bytes {2c, 2c + 1} of {p23, p01} below two zero bytes; symbol 4 would name the bytes 8 and 9 (a sign spread): it is selected away
	uint32_t const own = lp_perm(r.p23, r.p01, c * 0x0202u + 0x0C0C0100u);
	uint32_t const o = (c < 4u) ? own : 0u;
	// keep masks: the window {3, 3, 2, 2} + c over {FF FF FF 00 | FF FF FF FF} is zero in the low half for c = 0, in the high
	// half for c = 1; over {FF FF FF FF | FF 00 FF FF} for c = 2 and c = 3
	uint32_t const win = c * 0x01010101u + 0x02020303u;
	r.p01 &= lp_perm(0xFFFFFFFFu, 0x00FFFFFFu, win);
	r.p23 &= lp_perm(0xFFFF00FFu, 0xFFFFFFFFu, win);
	return o;
}

// A thread's E rows: dnew[e] as above, and the four tail maxima.  (On the device every dnew[e] is pinned to a vector register
// where it is made: it is needed only behind the step's barrier, and left alone the compiler sinks its select there and keeps
// the row's condition alive in an SGPR pair instead.)
template <int E>
FSEQ_LP_HD void local_pass_packed(uint32_t const (&d)[E], uint32_t const (&s)[E], uint32_t (&dnew)[E], uint32_t (&run)[4])
{
	PackedRuns r;
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (int e = 0; e < E; ++e)
	{
		dnew[e] = local_pass_packed_row(r, d[e], s[e]);
#if defined(__HIP_DEVICE_COMPILE__)
		asm volatile("" : "+v"(dnew[e]));
#endif
	}
	run[0] = r.p01 & 0xFFFFu; run[1] = r.p01 >> 16;
	run[2] = r.p23 & 0xFFFFu; run[3] = r.p23 >> 16;
}

} // namespace fseq
