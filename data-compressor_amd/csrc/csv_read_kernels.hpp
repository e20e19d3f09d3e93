// csv_read_kernels.hpp -- the reference's `decode csv` stage (ReadCSV, DCLib/src/csv.c:13-44) for gfx950 (MI355X).
//
// uint8 [C][stride] text with len[C] -> float32 [max_T][ld], channel c in column c, and per channel the number of values:
// the floats the reference writes for that text, bit for bit.  The splitting is csv.c:20-42 as it stands (a field ends at
// separator_char, at '\n' or at the last byte; only fields of column `column` are converted; '\n' resets the column; the
// LAST byte of the text is appended to a selected field whatever it is, csv.c:25-26).  The conversion is what glibc's
// strtof returns for the field in the C locale: leading white space, a sign, then the longest valid prefix of a decimal
// number (exponent only with a digit behind it), a hexadecimal one (0x, p exponent), inf / infinity, nan or
// nan(n-char-sequence) with glibc's payload rule; no conversion is +0.0f.  Rounding is to nearest, ties to even, on the
// EXACT decimal value.
//
// The conversion is INTEGER ONLY and the field is converted as its bytes arrive: there is no field buffer.  Per field a
// lane keeps the sign, up to 19 significant digits in a 64-bit register (two more registers for digits 20 .. 47), the
// number of decimals and the parser's state.
//   steady   -?digits[.digits], at most 19 significant digits and 27 decimals, no exponent: the value is W / 10^s =
//            W / 5^s x 2^-s with W < 2^64.  W is normalised to 64 bits, floor(W x 2^k / 5^s) is one 64 x 64 -> high 64
//            multiplication by a tabulated reciprocal of 5^s (at most one too small), the remainder is a wrapping 64-bit
//            multiply-subtract that corrects it and gives the sticky bit: 62 exact quotient bits or more, 25 are needed.
//   general  one divergent branch for everything else, right rather than fast: 20 .. 47 digits, exponents, hexadecimal,
//            inf / nan, white space.  A decimal D x 10^E outside [10^-47, 10^40) is 0 or inf without arithmetic; inside,
//            D x 10^max(E,0) < 2^157 is five 32-bit limbs, shifted left by 151 bits into ten (2^-150 is half the smallest
//            subnormal: no bit below it can matter but as sticky) and divided -E times by 10 (nine at a time by 10^9),
//            limb by limb.  The counterpart of the writer's 128-bit branch.
// One limit of the reference is NOT reproduced: its field buffer has 48 bytes (csv.c:11,18), so a selected field of 48 or
// more characters (the appended last byte counted, the terminator not) overruns it.  Such a channel gets
// ERR_INVALID_FORMAT, out_count = the values in front of that field, and stops there.
//
// Mapping: one lane = one channel, a wave = 64 channels (where a value lands depends on every line before it).
//   in    the lane's next CSVR_PIECES 16-byte pieces come by LDS-DMA into the lane's LDS column while the pieces before
//         them are consumed out of the other half, from registers, a byte per step.
//   conv  a finished steady field is not converted where it ends -- lanes end their fields at different bytes, and the
//         wave would pay for the conversion at nearly every byte -- but queued (W, decimals, sign) in the lane's LDS
//         column; every 8 bytes the wave converts what is queued, all lanes together.
//   out   values collect in a ring of CSVR_RING rows per lane in LDS; after every batch the rows every unfinished lane
//         has produced leave as whole rows of the wave (256 bytes).  A lane that runs more than the ring ahead of the
//         slowest writes its values straight to their rows until the wave has caught up (ends of channels, channels of
//         very different line lengths); a ragged wave's row store is masked.
// A channel with more than max_T values keeps counting without storing: ERR_MEMORY and out_count = the room it needs.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "dega_intrinsics.hpp"
#include "dega_launch.hpp"

#include <stddef.h>

namespace dg
{

constexpr uint32_t CSVR_BLOCK = 256;     // lanes = adjacent channels per workgroup
constexpr uint32_t CSVR_PIECES = 2;      // 16-byte pieces per lane and batch; one batch is in flight while one is consumed
constexpr uint32_t CSVR_BATCH = 16u * CSVR_PIECES;
constexpr uint32_t CSVR_RING = 16;       // rows a lane may be ahead of the rows stored
constexpr uint32_t CSVR_PEND = 8;        // fields queued per lane between two conversions (one can end per byte)
constexpr uint32_t CSVR_FIELD_MAX = 47;  // characters of a selected field the reference can hold (csv.c:11)
constexpr uint32_t CSVR_STEADY_DECIMALS = 27; // 5^27 < 2^63
constexpr int32_t CSVR_OK = 0, CSVR_ERR_INVALID_VALUE = -1, CSVR_ERR_INVALID_FORMAT = -3, CSVR_ERR_MEMORY = -6;

struct CsvReadArgs
{
  const uint8_t *text;   // [C][stride], 16-byte aligned
  size_t stride;         // a multiple of 16, at most 0x7FFFFFF0
  const uint64_t *len;   // [C]
  size_t C;
  uint32_t column;       // 1 ..; 0: beyond every line (a column of 2^32 or more)
  uint32_t sep;          // separator_char
  float *v;              // [max_T][ld]
  size_t max_T, ld;
  uint64_t *out_count;   // [C]
  int32_t *err;          // [C]
};

// {5^s, floor(2^(63 + bits(5^s)) / 5^s)}: the divisor of the steady path and its reciprocal, normalised to 64 bits
constexpr uint64_t CSVR_POW5[CSVR_STEADY_DECIMALS + 1][2] = {
  {0x0000000000000001ull, 0x0000000000000000ull}, // (s = 0 does not divide)
  {0x0000000000000005ull, 0xCCCCCCCCCCCCCCCCull},
  {0x0000000000000019ull, 0xA3D70A3D70A3D70Aull},
  {0x000000000000007Dull, 0x83126E978D4FDF3Bull},
  {0x0000000000000271ull, 0xD1B71758E219652Bull},
  {0x0000000000000C35ull, 0xA7C5AC471B478423ull},
  {0x0000000000003D09ull, 0x8637BD05AF6C69B5ull},
  {0x000000000001312Dull, 0xD6BF94D5E57A42BCull},
  {0x000000000005F5E1ull, 0xABCC77118461CEFCull},
  {0x00000000001DCD65ull, 0x89705F4136B4A597ull},
  {0x00000000009502F9ull, 0xDBE6FECEBDEDD5BEull},
  {0x0000000002E90EDDull, 0xAFEBFF0BCB24AAFEull},
  {0x000000000E8D4A51ull, 0x8CBCCC096F5088CBull},
  {0x0000000048C27395ull, 0xE12E13424BB40E13ull},
  {0x000000016BCC41E9ull, 0xB424DC35095CD80Full},
  {0x000000071AFD498Dull, 0x901D7CF73AB0ACD9ull},
  {0x0000002386F26FC1ull, 0xE69594BEC44DE15Bull},
  {0x000000B1A2BC2EC5ull, 0xB877AA3236A4B449ull},
  {0x000003782DACE9D9ull, 0x9392EE8E921D5D07ull},
  {0x00001158E460913Dull, 0xEC1E4A7DB69561A5ull},
  {0x000056BC75E2D631ull, 0xBCE5086492111AEAull},
  {0x0001B1AE4D6E2EF5ull, 0x971DA05074DA7BEEull},
  {0x000878678326EAC9ull, 0xF1C90080BAF72CB1ull},
  {0x002A5A058FC295EDull, 0xC16D9A0095928A27ull},
  {0x00D3C21BCECCEDA1ull, 0x9ABE14CD44753B52ull},
  {0x0422CA8B0A00A425ull, 0xF79687AED3EEC551ull},
  {0x14ADF4B7320334B9ull, 0xC612062576589DDAull},
  {0x6765C793FA10079Dull, 0x9E74D1B791E07E48ull},
};

DG_DEV uint64_t csvr_mulhi64(uint64_t a, uint64_t b)
{
#if defined(DEGA_SIM)
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#else
  return __umul64hi(a, b);
#endif
}

DG_DEV uint32_t csvr_clz64(uint64_t x) // x != 0
{
  return (uint32_t)__builtin_clzll(x);
}

// The float nearest to w x 2^(e - 63) (bit 63 of w set; `sticky`: the exact value is a little more), ties to even,
// subnormals and overflow included; without the sign.
// hex: glibc's quirk for hexadecimal input is part of the format.  Its round_and_return takes 24 bits, the bit behind them
// and "more"; when the result is subnormal it shifts the 24 down again and folds what was behind them into "more" --
// except that bit itself, which is lost: 0x1.000001p-150 reads as 0, not as the smallest subnormal.  (A decimal field of
// 47 characters cannot show it: its value is never that short in binary.)
DG_DEV uint32_t csvr_round(uint64_t w, int32_t e, bool sticky, bool hex)
{
  if (e > 127)
    return 0x7F800000u;
  if (e < -150) // below half of the smallest subnormal
    return 0u;
  if (hex && e < -126)
    w &= ~(1ull << 39);
  const uint32_t keep = e >= -126 ? 24u : (uint32_t)(e + 150); // bits of w that stay: 24 .. 0
  const uint32_t shift = 64u - keep;                             // 40 .. 64
  uint32_t mant = keep != 0 ? (uint32_t)(w >> shift) : 0u;
  const uint32_t round_bit = (uint32_t)(w >> (shift - 1u)) & 1u;
  const bool below = sticky || (w & ((1ull << (shift - 1u)) - 1ull)) != 0;
  mant += round_bit & ((below ? 1u : 0u) | (mant & 1u));
  // (the hidden bit of a normal number adds one to the exponent field, and so does a carry out of the mantissa)
  const uint32_t bits = (e >= -126 ? (uint32_t)(e + 126) << 23 : 0u) + mant;
  return bits >= 0x7F800000u ? 0x7F800000u : bits;
}

// W / 10^s for W < 2^64 and s <= CSVR_STEADY_DECIMALS: never subnormal, never infinite.  pow5 = {5^s, its reciprocal}.
DG_DEV uint32_t csvr_steady(uint64_t W, uint32_t s, uint64_t pow5, uint64_t recip)
{
  if (W == 0)
    return 0u;
  const uint32_t lz = csvr_clz64(W);
  const uint64_t Wn = W << lz;
  uint64_t q = Wn;
  bool sticky = false;
  int32_t e = 63 - (int32_t)lz;
  if (s != 0)
  {
    // x = Wn x 2^(L-1) / 5^s with L = bits(5^s) lies in (2^62, 2^64); mulhi gives floor(x) or one less
    const uint32_t L = 64u - csvr_clz64(pow5);
    q = csvr_mulhi64(Wn, recip);
    uint64_t rem = (Wn << (L - 1u)) - q * pow5; // exact: below 2 x 5^s, the bits above 64 cancel
    if (rem >= pow5)
    {
      q++;
      rem -= pow5;
    }
    sticky = rem != 0;
    const uint32_t up = (uint32_t)(~q >> 63); // 1 when bit 63 of q is clear (the bit shifted in is covered by sticky)
    q <<= up;
    e = 64 - (int32_t)up - (int32_t)lz - (int32_t)s - (int32_t)L;
  }
  const uint32_t mant = (uint32_t)(q >> 40);
  const uint32_t round_bit = (uint32_t)(q >> 39) & 1u;
  const bool below = sticky || (q & ((1ull << 39) - 1ull)) != 0;
  return ((uint32_t)(e + 126) << 23) + mant + (round_bit & ((below ? 1u : 0u) | (mant & 1u)));
}

// ---- one field in the making -------------------------------------------------------------------------------------------
enum : uint32_t
{
  CSVR_START = 0, // white space may still come
  CSVR_SIGNED,    // a sign has come
  CSVR_ZERO,      // a single '0': an 'x' may follow
  CSVR_INT,       // decimal digits
  CSVR_FRAC,      // decimal digits behind the point (a number already)
  CSVR_DOT0,      // '.' without a digit in front: a number only if a digit follows
  CSVR_EPEND,     // e / p: counts only if a digit follows, behind an optional sign
  CSVR_ESIGN,
  CSVR_EXP,
  CSVR_HX,        // "0x": so far the number 0
  CSVR_HINT,
  CSVR_HDOT0,     // "0x."
  CSVR_HFRAC,
  CSVR_WINF,      // i, in
  CSVR_WNAN,      // n, na
  CSVR_NANOPEN,   // nan: a '(' may follow
  CSVR_NANSEQ,    // nan(...
  CSVR_DONE       // the rest of the field is ignored
};
enum : uint32_t { CSVR_NONE = 0, CSVR_DEC, CSVR_HEX, CSVR_INF, CSVR_NAN };

struct CsvrField
{
  uint64_t w0, w1, w2; // decimal: significant digits 1..19, 20..38, 39..; hex: 16 digits in w0, integer digits dropped in w1;
                       // nan(: the payload so far in w0
  uint32_t st, kind;
  uint32_t nd;         // significant digits so far (from the first that is not 0); WINF/WNAN: letters matched; NANSEQ: see below
  uint32_t fdig;       // digits behind the point
  uint32_t ev;         // exponent digits' value, saturated; NAN: the bit pattern
  uint32_t flen;       // characters of the field
  uint32_t neg, eneg;
  uint32_t sticky;     // hex: a non-zero digit was dropped; nan(: the payload overflowed 64 bits
  DG_DEV void reset()
  {
    w0 = w1 = w2 = 0;
    st = CSVR_START;
    kind = CSVR_NONE;
    nd = fdig = ev = flen = neg = eneg = sticky = 0;
  }
};

DG_DEV void csvr_add_dec(CsvrField &f, uint32_t d, bool frac)
{
  if ((f.nd | d) != 0) // (zeros in front are not significant)
  {
    if (f.nd < 19u)
      f.w0 = f.w0 * 10u + d;
    else if (f.nd < 38u)
      f.w1 = f.w1 * 10u + d;
    else
      f.w2 = f.w2 * 10u + d; // (a field has at most 47 characters: at most 9 digits here)
    f.nd++;
  }
  f.fdig += frac ? 1u : 0u;
}

DG_DEV void csvr_add_hex(CsvrField &f, uint32_t d, bool frac)
{
  if ((f.nd | d) == 0)
    f.fdig += frac ? 1u : 0u;
  else if (f.nd < 16u)
  {
    f.w0 = (f.w0 << 4) | d;
    f.nd++;
    f.fdig += frac ? 1u : 0u;
  }
  else
  {
    f.sticky |= d != 0 ? 1u : 0u;
    f.w1 += frac ? 0u : 1u;
  }
}

// nan(n-char-sequence): glibc takes strtoull(sequence, &end, 0) as the payload when the whole sequence is a number.
// f.nd: 0 nothing yet, 1 a single '0', 2 octal, 3 "0x", 4 hexadecimal, 5 decimal, 6 not a number
DG_DEV void csvr_payload(CsvrField &f, uint32_t d, uint32_t hx, uint32_t lc)
{
  uint32_t base = 0;
  switch (f.nd)
  {
  case 0:
    if (d == 0)
      f.nd = 1;
    else if (d < 10u)
      f.nd = 5, base = 10;
    else
      f.nd = 6;
    break;
  case 1:
    if (lc == 0x78u)
      f.nd = 3;
    else if (d < 8u)
      f.nd = 2, base = 8;
    else
      f.nd = 6;
    break;
  case 2:
    if (d < 8u)
      base = 8;
    else
      f.nd = 6;
    break;
  case 3:
  case 4:
    if (hx < 16u)
      f.nd = 4, base = 16, d = hx;
    else
      f.nd = 6;
    break;
  case 5:
    if (d < 10u)
      base = 10;
    else
      f.nd = 6;
    break;
  default:
    break;
  }
  if (base != 0)
  {
    const uint64_t lo = f.w0 * base;
    if (csvr_mulhi64(f.w0, base) != 0 || lo + d < lo)
      f.sticky = 1; // strtoull returns ULLONG_MAX and reads on
    f.w0 = lo + d;
  }
}

// every character the steady form does not take
DG_DEV void csvr_feed_slow(CsvrField &f, uint32_t ch)
{
  const uint32_t d = ch - 0x30u, lc = ch | 0x20u;
  const bool digit = d < 10u;
  const uint32_t hx = digit ? d : ((lc >= 0x61u && lc <= 0x66u) ? lc - 0x61u + 10u : 16u);
  const bool sign = ch == 0x2Bu || ch == 0x2Du;
  switch (f.st)
  {
  case CSVR_START:
    if (ch == 0x20u || (ch >= 0x09u && ch <= 0x0Du))
      break;
    if (sign)
    {
      f.neg = ch == 0x2Du ? 1u : 0u;
      f.st = CSVR_SIGNED;
      break;
    }
    [[fallthrough]];
  case CSVR_SIGNED:
    if (digit)
    {
      f.kind = CSVR_DEC;
      f.st = d != 0 ? CSVR_INT : CSVR_ZERO;
      csvr_add_dec(f, d, false);
    }
    else if (ch == 0x2Eu)
      f.st = CSVR_DOT0;
    else if (lc == 0x69u) // i
      f.st = CSVR_WINF, f.nd = 1;
    else if (lc == 0x6Eu) // n
      f.st = CSVR_WNAN, f.nd = 1;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_ZERO:
    if (lc == 0x78u) // x
    {
      f.st = CSVR_HX;
      break;
    }
    [[fallthrough]];
  case CSVR_INT:
    if (digit)
    {
      f.st = CSVR_INT;
      csvr_add_dec(f, d, false);
    }
    else if (ch == 0x2Eu)
      f.st = CSVR_FRAC;
    else if (lc == 0x65u) // e
      f.st = CSVR_EPEND;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_DOT0:
    if (digit)
    {
      f.kind = CSVR_DEC;
      f.st = CSVR_FRAC;
      csvr_add_dec(f, d, true);
    }
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_FRAC:
    if (digit)
      csvr_add_dec(f, d, true);
    else if (lc == 0x65u)
      f.st = CSVR_EPEND;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_EPEND:
    if (sign)
    {
      f.eneg = ch == 0x2Du ? 1u : 0u;
      f.st = CSVR_ESIGN;
      break;
    }
    [[fallthrough]];
  case CSVR_ESIGN:
    if (digit)
      f.st = CSVR_EXP, f.ev = d;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_EXP:
    if (digit)
      f.ev = f.ev < 100000u ? f.ev * 10u + d : f.ev; // (saturated: beyond every float either way)
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_HX:
    if (hx < 16u)
    {
      f.kind = CSVR_HEX;
      f.st = CSVR_HINT;
      csvr_add_hex(f, hx, false);
    }
    else if (ch == 0x2Eu)
      f.st = CSVR_HDOT0;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_HINT:
    if (hx < 16u)
      csvr_add_hex(f, hx, false);
    else if (ch == 0x2Eu)
      f.st = CSVR_HFRAC;
    else if (lc == 0x70u) // p
      f.st = CSVR_EPEND;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_HDOT0:
    if (hx < 16u)
    {
      f.kind = CSVR_HEX;
      f.st = CSVR_HFRAC;
      csvr_add_hex(f, hx, true);
    }
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_HFRAC:
    if (hx < 16u)
      csvr_add_hex(f, hx, true);
    else if (lc == 0x70u)
      f.st = CSVR_EPEND;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_WINF: // "inf" is all it takes: "infinity" and every prefix of it read the same
    if (lc == (f.nd == 1u ? 0x6Eu : 0x66u))
    {
      if (++f.nd == 3u)
        f.kind = CSVR_INF, f.st = CSVR_DONE;
    }
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_WNAN:
    if (lc == (f.nd == 1u ? 0x61u : 0x6Eu))
    {
      if (++f.nd == 3u)
        f.kind = CSVR_NAN, f.st = CSVR_NANOPEN, f.ev = 0x7FC00000u;
    }
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_NANOPEN:
    if (ch == 0x28u)
      f.st = CSVR_NANSEQ, f.nd = 0, f.w0 = 0, f.sticky = 0;
    else
      f.st = CSVR_DONE;
    break;
  case CSVR_NANSEQ:
    if (ch == 0x29u)
    {
      if (f.nd != 3u && f.nd != 6u) // the whole sequence was a number (the empty one is 0)
        f.ev |= f.sticky != 0 ? 0x3FFFFFu : (uint32_t)f.w0 & 0x3FFFFFu;
      f.st = CSVR_DONE;
    }
    else if (digit || (lc >= 0x61u && lc <= 0x7Au) || ch == 0x5Fu)
      csvr_payload(f, d, hx, lc);
    else
      f.st = CSVR_DONE;
    break;
  default:
    break;
  }
}

// L = L x mult + add over five limbs (the product stays below 2^160)
DG_DEV void csvr_limbs_muladd(uint32_t (&L)[5], uint32_t mult, uint32_t add)
{
  uint64_t carry = add;
#pragma unroll
  for (uint32_t i = 0; i < 5; i++)
  {
    const uint64_t cur = (uint64_t)L[i] * mult + carry;
    L[i] = (uint32_t)cur;
    carry = cur >> 32;
  }
}

DG_DEV void csvr_limbs_add64(uint32_t (&L)[5], uint64_t x)
{
  uint64_t cur = (uint64_t)L[0] + (uint32_t)x;
  L[0] = (uint32_t)cur;
  cur = (cur >> 32) + L[1] + (x >> 32);
  L[1] = (uint32_t)cur;
#pragma unroll
  for (uint32_t i = 2; i < 5; i++)
  {
    cur = (cur >> 32) + L[i];
    L[i] = (uint32_t)cur;
  }
}

template <uint32_t DIV>
DG_DEV bool csvr_limbs_div(uint32_t (&X)[10]) // X = floor(X / DIV); returns whether something was left
{
  uint64_t r = 0;
#pragma unroll
  for (uint32_t i = 10; i-- > 0;)
  {
    const uint64_t cur = (r << 32) | X[i];
    const uint64_t q = cur / DIV;
    X[i] = (uint32_t)q;
    r = cur - q * DIV;
  }
  return r != 0;
}

// the float of a finished field, sign included: everything the steady form is not
DG_DEV uint32_t csvr_finish(const CsvrField &f)
{
  const uint32_t sign = f.neg << 31;
  if (f.kind == CSVR_NONE)
    return 0u; // no conversion: +0.0f even behind a '-'
  if (f.kind == CSVR_INF)
    return sign | 0x7F800000u;
  if (f.kind == CSVR_NAN)
    return sign | f.ev;
  if (f.nd == 0)
    return sign;
  const int32_t ex = f.eneg != 0 ? -(int32_t)f.ev : (int32_t)f.ev; // (0 without exponent digits)
  if (f.kind == CSVR_HEX)
  {
    const uint32_t lz = csvr_clz64(f.w0);
    const int32_t e = 63 - (int32_t)lz + 4 * ((int32_t)(uint32_t)f.w1 - (int32_t)f.fdig) + ex;
    return sign | csvr_round(f.w0 << lz, e, f.sticky != 0, true);
  }
  // D x 10^E, D of nd digits
  const int32_t E = ex - (int32_t)f.fdig, nd = (int32_t)f.nd;
  if (nd + E <= -47) // below 10^-47 < 2^-150
    return sign;
  if (nd - 1 + E >= 40) // 10^40 and above
    return sign | 0x7F800000u;
  uint32_t L[5] = {(uint32_t)f.w0, (uint32_t)(f.w0 >> 32), 0u, 0u, 0u};
  if (f.nd > 19u) // D = w0 x 10^j + w1, j digits in w1
  {
    for (uint32_t j = (f.nd < 38u ? f.nd : 38u) - 19u; j != 0; j--)
      csvr_limbs_muladd(L, 10u, 0u);
    csvr_limbs_add64(L, f.w1);
  }
  if (f.nd > 38u) // and again with the at most 9 digits in w2
  {
    for (uint32_t j = f.nd - 38u; j != 0; j--)
      csvr_limbs_muladd(L, 10u, 0u);
    csvr_limbs_add64(L, f.w2);
  }
  for (int32_t k = 0; k < E; k++) // (E <= 40 - nd: the product stays below 10^40 < 2^133)
    csvr_limbs_muladd(L, 10u, 0u);
  // X = D x 2^151: four limbs and 23 bits up
  uint32_t X[10];
#pragma unroll
  for (uint32_t i = 0; i < 4; i++)
    X[i] = 0;
#pragma unroll
  for (uint32_t i = 0; i < 6; i++)
    X[4 + i] = (i < 5 ? L[i] << 23 : 0u) | (i > 0 ? L[i - 1] >> 9 : 0u);
  bool sticky = false;
  int32_t m = E < 0 ? -E : 0; // at most 93
  for (; m >= 9; m -= 9)
    sticky |= csvr_limbs_div<1000000000u>(X);
  for (; m > 0; m--)
    sticky |= csvr_limbs_div<10u>(X);
  // the value is X x 2^-151 (and a little more when sticky): its 64 leading bits
  int32_t top = -1;
#pragma unroll
  for (int32_t i = 0; i < 10; i++)
    top = X[i] != 0 ? i : top;
  if (top < 0) // below 2^-151
    return sign;
  uint32_t a = 0, b = 0, c = 0;
#pragma unroll
  for (int32_t i = 0; i < 10; i++)
  {
    a |= i == top ? X[i] : 0u;
    b |= i == top - 1 ? X[i] : 0u;
    c |= i == top - 2 ? X[i] : 0u;
    sticky |= i < top - 2 && X[i] != 0;
  }
  const uint32_t lz = clz32(a);
  uint64_t w = (((uint64_t)a << 32) | b) << lz;
  if (lz != 0)
  {
    w |= c >> (32u - lz);
    sticky |= (uint32_t)(c << lz) != 0;
  }
  else
    sticky |= c != 0;
  return sign | csvr_round(w, 32 * top + 31 - (int32_t)lz - 151, sticky, false);
}

__global__ void __launch_bounds__(256) dega_csv_read_kernel(const CsvReadArgs a)
{
  // pieces on their way: [half][piece][wave][lane][4 dwords] -- what one LDS-DMA load of a wave fills is 1 KiB
  __shared__ uint32_t pieces[2 * CSVR_PIECES * CSVR_BLOCK * 4];
  __shared__ uint32_t ring[CSVR_RING * CSVR_BLOCK];     // values on their way out: [row % CSVR_RING][lane]
  __shared__ uint32_t pend_lo[CSVR_PEND * CSVR_BLOCK];  // fields to convert: W, or the finished float
  __shared__ uint32_t pend_hi[CSVR_PEND * CSVR_BLOCK];
  __shared__ uint32_t pend_meta[CSVR_PEND * CSVR_BLOCK]; // decimals | sign << 8 | finished << 9
  __shared__ uint64_t pow5[2 * (CSVR_STEADY_DECIMALS + 1)];
  if (threadIdx.x <= CSVR_STEADY_DECIMALS)
  {
    pow5[2 * threadIdx.x] = CSVR_POW5[threadIdx.x][0];
    pow5[2 * threadIdx.x + 1] = CSVR_POW5[threadIdx.x][1];
  }
  __syncthreads();

  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave0 = wave_uniform(tid & ~63u);
  const size_t c = (size_t)blockIdx.x * CSVR_BLOCK + tid;
  const bool live = c < a.C;
  const uint32_t stride = (uint32_t)a.stride;
  const uint8_t *const src = a.text + (live ? c : a.C - 1) * a.stride; // (a lane without a channel reads the last one's: valid addresses)
  const uint64_t len64 = live ? a.len[c] : 0;
  const bool too_long = len64 > a.stride;
  const uint32_t n = too_long ? 0u : (uint32_t)len64;
  const uint32_t T32 = a.max_T < 0xFFFFFFFFu ? (uint32_t)a.max_T : 0xFFFFFFFFu;
  const uint32_t column = a.column, sep = a.sep & 0xFFu;
  float *const dst = a.v + (live ? c : 0);

  CsvrField f;
  f.reset();
  uint32_t col = 1;
  uint32_t t = 0;                 // values so far (queued ones not yet)
  uint32_t queued = 0, drained = 0;
  uint32_t rows_stored = 0;       // rows below it are in memory for every lane that has them (wave uniform)
  uint32_t ring_end = CSVR_RING;  // this lane's rows below it go through the ring; t > ring_end: it is writing straight
  int32_t status = too_long ? CSVR_ERR_INVALID_VALUE : CSVR_OK;
  bool stopped = false;

  auto put = [&](uint32_t bits) {
    if (t < T32)
    {
      if (t < ring_end)
        ring[(t % CSVR_RING) * CSVR_BLOCK + tid] = bits;
      else
        reinterpret_cast<uint32_t *>(dst)[(size_t)t * a.ld] = bits;
    }
    t++;
  };
  auto convert_queued = [&]() { // all lanes together: what the last bytes have queued
    const uint32_t most = wave_max_u32(queued - drained);
    for (uint32_t k = 0; k < most; k++)
    {
      if (drained != queued)
      {
        const uint32_t slot = (drained % CSVR_PEND) * CSVR_BLOCK + tid;
        const uint32_t meta = pend_meta[slot];
        const uint64_t W = ((uint64_t)pend_hi[slot] << 32) | pend_lo[slot];
        uint32_t bits = (uint32_t)W;
        if ((meta & 0x200u) == 0)
        {
          const uint32_t s = meta & 0xFFu;
          bits = csvr_steady(W, s, pow5[2 * s], pow5[2 * s + 1]) | ((meta & 0x100u) << 23);
        }
        put(bits);
        drained++;
      }
    }
  };
  auto step = [&](uint32_t ch, bool last) { // csv.c:22-41 for one character
    const bool end = ch == sep || ch == 0x0Au || last;
    const bool selected = col == column;
    if (selected && (!end || last))
    {
      f.flen++;
      const uint32_t d = ch - 0x30u;
      if (d < 10u && f.st <= CSVR_FRAC && f.nd < 19u) // the steady form: a digit of a decimal number
      {
        f.kind = CSVR_DEC;
        f.st = f.st == CSVR_FRAC ? CSVR_FRAC : ((f.st <= CSVR_SIGNED && d == 0) ? CSVR_ZERO : CSVR_INT);
        f.w0 = f.w0 * 10u + d;
        f.nd += (f.nd | d) != 0 ? 1u : 0u;
        f.fdig += f.st == CSVR_FRAC ? 1u : 0u;
      }
      else if (ch == 0x2Eu && (f.st == CSVR_ZERO || f.st == CSVR_INT))
        f.st = CSVR_FRAC;
      else
        csvr_feed_slow(f, ch);
      if (f.flen > CSVR_FIELD_MAX) // the reference's buffer overruns here: not reproduced
      {
        status = CSVR_ERR_INVALID_FORMAT;
        stopped = true;
        return;
      }
    }
    if (end)
    {
      if (selected)
      {
        const uint32_t slot = (queued % CSVR_PEND) * CSVR_BLOCK + tid;
        uint64_t W = f.w0;
        uint32_t meta = f.fdig | (f.neg << 8);
        if (!(f.st >= CSVR_ZERO && f.st <= CSVR_FRAC && f.nd <= 19u && f.fdig <= CSVR_STEADY_DECIMALS))
        {
          W = csvr_finish(f);
          meta = 0x200u;
        }
        pend_lo[slot] = (uint32_t)W;
        pend_hi[slot] = (uint32_t)(W >> 32);
        pend_meta[slot] = meta;
        queued++;
        f.reset();
      }
      col++;
    }
    if (ch == 0x0Au)
      col = 1;
  };
  auto fetch = [&](uint32_t batch, uint32_t half) { // the pieces of `batch` into `half`, clamped to the row
    wait_lds(); // what was read out of this half is out of it
#pragma unroll
    for (uint32_t u = 0; u < CSVR_PIECES; u++)
    {
      const uint32_t at = batch * CSVR_BATCH + 16u * u;
      const uint32_t off = at < stride - 16u ? at : stride - 16u;
      dma_x4_to_lds(reinterpret_cast<const int32_t *>(src + off), pieces + ((half * CSVR_PIECES + u) * CSVR_BLOCK + wave0) * 4u, lane);
    }
  };

  const uint32_t batches = wave_max_u32((n + CSVR_BATCH - 1u) / CSVR_BATCH); // (n <= 0x7FFFFFF0)
  if (batches != 0)
    fetch(0, 0);
  uint32_t half = 0;
  for (uint32_t b = 0; b < batches; b++, half ^= 1u)
  {
    wait_vector_memory(); // this batch has landed (asked for one batch ago)
    if (b + 1u < batches)
      fetch(b + 1u, half ^ 1u);
#pragma unroll 1
    for (uint32_t u = 0; u < 2u * CSVR_PIECES; u++) // 8 bytes at a time
    {
      const uint32_t *const p = pieces + ((half * CSVR_PIECES + (u >> 1)) * CSVR_BLOCK + tid) * 4u + 2u * (u & 1u);
      uint64_t word = (uint64_t)peer_load(p) | ((uint64_t)peer_load(p + 1) << 32);
      uint32_t pos = b * CSVR_BATCH + 8u * u;
#pragma unroll 1
      for (uint32_t k = 0; k < 8u; k++, pos++, word >>= 8)
        if (pos < n && !stopped)
          step((uint32_t)word & 0xFFu, pos + 1u == n);
      convert_queued();
    }
    // ---- rows every unfinished lane has produced leave the ring ----
    const bool finished = stopped || (uint64_t)(b + 1u) * CSVR_BATCH >= n;
    uint32_t upto = wave_min_u32(finished ? 0xFFFFFFFFu : t);
    if (upto == 0xFFFFFFFFu) // every lane has finished: all that is left
      upto = wave_max_u32(t);
    const uint32_t mine = t < ring_end ? t : ring_end; // (and below T32: put() keeps later rows out of the ring)
    for (uint32_t r = rows_stored; r < upto && r < T32; r++)
      if (r < mine && r < T32)
        reinterpret_cast<uint32_t *>(dst)[(size_t)r * a.ld] = ring[(r % CSVR_RING) * CSVR_BLOCK + tid];
    rows_stored = upto > rows_stored ? upto : rows_stored;
    if (t <= ring_end || rows_stored >= t) // not writing straight, or caught up with
      ring_end = rows_stored + CSVR_RING < rows_stored ? 0xFFFFFFFFu : rows_stored + CSVR_RING;
  }
  if (!live)
    return;
  a.out_count[c] = t;
  a.err[c] = status != CSVR_OK ? status : (t > a.max_T ? CSVR_ERR_MEMORY : CSVR_OK);
}

// ---- host side: how the kernel is launched (dega_launch.hpp); one instantiation ----------------------------------------------
inline CsvReadArgs csv_read_args(const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column, int separator_char, float *v, size_t max_T,
                                 size_t ld, uint64_t *out_count, int32_t *err)
{
  CsvReadArgs a;
  a.text = text;
  a.stride = stride;
  a.len = len;
  a.C = C;
  a.column = column <= 0xFFFFFFFFu ? (uint32_t)column : 0u; // (no line has 2^32 fields: such a column selects nothing)
  a.sep = (uint32_t)separator_char;
  a.v = v;
  a.max_T = max_T;
  a.ld = ld;
  a.out_count = out_count;
  a.err = err;
  return a;
}

template <typename L>
inline bool launch(const CsvReadArgs &a, L &&launch_one)
{
  const size_t gx = (a.C + CSVR_BLOCK - 1) / CSVR_BLOCK;
  if (gx > LAUNCH_MAX_GX)
    return false;
  launch_one(dega_csv_read_kernel, LaunchGrid{(uint32_t)gx, 1}, CSVR_BLOCK, a);
  return true;
}

} // namespace dg
