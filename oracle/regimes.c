/* regimes.c -- helper of tests/encoder_regimes_common.py: an instrumented replay of the reference's arithmetic coder and a
 * steerer that builds input series on which the coder's rare paths are the common ones.
 *
 * TEST INFRASTRUCTURE ONLY, like everything under oracle/.  Written apart from dega_oracle.c on purpose: the replay is
 * trusted only after its stream has been compared bit for bit with the oracle's (the Python side asserts that on every
 * channel), and only then are its counts -- pending bits, rows, model states -- used.
 *
 * The coder (DCLib/src/bac.c, Witten/Neal/Cleary): a 16-bit interval [start, end], three symbols by index -- 1 the more
 * probable binary symbol, 2 the less probable one, 3 EOF with a count of 1 --, index i takes
 * [start + range * cum[i] / cum[0], start + range * cum[i - 1] / cum[0] - 1].  An interval inside [Q, 3Q) is widened
 * about the half point and a bit is owed ("pending"); the next bit that does get out settles all the owed ones as its
 * inverse.  A `1` out after p owed bits is what a coder that writes the owed bits at once as `0 1 1 .. 1` sees as a CARRY
 * through p ones; a `0` out leaves the p ones standing.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define RG_HALF 0x8000u
#define RG_QUARTER 0x4000u
#define RG_THREE_QUARTERS 0xC000u
#define RG_MAX_FREQUENCY 0x3FFFu

typedef struct rg_model
{
  unsigned sym2idx[2];
  unsigned idx2sym[4];
  uint32_t freq[4], cum[4];
} rg_model_t;

typedef struct rg_coder
{
  uint32_t start, end; /* 16 bits each */
  uint64_t pending;
} rg_coder_t;

/* what the replay records; any pointer may be NULL */
typedef struct rg_sink
{
  uint8_t *bits; /* the stream, one bit per byte */
  size_t nbits, cap;
  uint32_t *ev_pos, *ev_pend, *ev_sym; /* per emit event: position of its first bit, owed bits it settles, symbol being coded */
  uint8_t *ev_bit;
  size_t nev, ev_cap;
  int overflow;
  size_t sym; /* index of the symbol being coded */
} rg_sink_t;

static void model_init(rg_model_t *m)
{
  m->sym2idx[0] = 1;
  m->sym2idx[1] = 2;
  m->idx2sym[0] = 0;
  m->idx2sym[1] = 0;
  m->idx2sym[2] = 1;
  m->idx2sym[3] = 0;
  m->freq[0] = 0;
  m->freq[1] = m->freq[2] = m->freq[3] = 1;
  m->cum[0] = 3;
  m->cum[1] = 2;
  m->cum[2] = 1;
  m->cum[3] = 0;
}

/* bac.c:54-81.  Returns 1 for a halving of the counts, 2 for an exchange of the two symbols' indices, 3 for both. */
static int model_update(rg_model_t *m, unsigned last)
{
  int what = 0;
  unsigned i;
  if (m->cum[0] == RG_MAX_FREQUENCY)
  {
    uint32_t c = 0;
    for (i = 4; i-- != 0;)
    {
      m->freq[i] = (m->freq[i] + 1) / 2;
      m->cum[i] = c;
      c += m->freq[i];
    }
    what |= 1;
  }
  for (i = last; m->freq[i] == m->freq[i - 1]; i--)
    ;
  if (i < last)
  {
    const unsigned a = m->idx2sym[i], b = m->idx2sym[last];
    m->idx2sym[i] = b;
    m->idx2sym[last] = a;
    m->sym2idx[a] = last;
    m->sym2idx[b] = i;
    what |= 2;
  }
  m->freq[i]++;
  while (i-- > 0)
    m->cum[i]++;
  return what;
}

static void sink_put(rg_sink_t *s, unsigned bit)
{
  if (s->bits != NULL)
  {
    if (s->nbits < s->cap)
      s->bits[s->nbits] = (uint8_t)bit;
    else
      s->overflow = 1;
  }
  s->nbits++;
}

static void emit(rg_coder_t *e, rg_sink_t *s, unsigned bit)
{
  if (s != NULL)
  {
    if (s->ev_pos != NULL)
    {
      if (s->nev < s->ev_cap)
      {
        s->ev_pos[s->nev] = (uint32_t)s->nbits;
        s->ev_pend[s->nev] = (uint32_t)e->pending;
        s->ev_sym[s->nev] = (uint32_t)s->sym;
        s->ev_bit[s->nev] = (uint8_t)bit;
      }
      else
        s->overflow = 1;
    }
    s->nev++;
    sink_put(s, bit);
    for (uint64_t k = 0; k < e->pending; k++)
      sink_put(s, !bit);
  }
  e->pending = 0;
}

/* the sub-interval of index idx (bac.c:109-111), not yet widened */
static void narrow(const rg_coder_t *e, const rg_model_t *m, unsigned idx, uint32_t *start, uint32_t *end)
{
  const uint64_t range = (uint64_t)(e->end - e->start) + 1;
  *end = (e->start + (uint32_t)((range * m->cum[idx - 1]) / m->cum[0]) - 1) & 0xFFFFu;
  *start = (e->start + (uint32_t)((range * m->cum[idx]) / m->cum[0])) & 0xFFFFu;
}

static void encode_symbol(rg_coder_t *e, const rg_model_t *m, unsigned idx, rg_sink_t *s) /* bac.c:107-139 */
{
  narrow(e, m, idx, &e->start, &e->end);
  for (;;)
  {
    if (e->end < RG_HALF)
      emit(e, s, 0);
    else if (e->start >= RG_HALF)
    {
      emit(e, s, 1);
      e->start -= RG_HALF;
      e->end -= RG_HALF;
    }
    else if (e->start >= RG_QUARTER && e->end < RG_THREE_QUARTERS)
    {
      e->pending++;
      e->start -= RG_QUARTER;
      e->end -= RG_QUARTER;
    }
    else
      break;
    e->start = (2 * e->start) & 0xFFFFu;
    e->end = (2 * e->end + 1) & 0xFFFFu;
  }
}

/* the signed exp-Golomb codeword of one difference (seg.c:11-28), one bit per byte, at most 65 -> its length */
static unsigned codeword(int64_t v, uint8_t *bits)
{
  const uint64_t w = (v > 0 ? 2 * (uint64_t)v - 1 : 2 * (uint64_t)(-v)) + 1;
  unsigned p = 0, n = 0;
  while ((w >> (p + 1)) != 0)
    p++;
  memset(bits, 0, p);
  n = p;
  for (unsigned k = p + 1; k-- != 0;)
    bits[n++] = (uint8_t)((w >> k) & 1u);
  return n;
}

/* The seg stream of a series (diff.c:15-20, seg.c:11-28), one bit per byte; the samples are the 32 bits of x, unsigned.
 * row_end[t]: bits after row t.  Returns the number of bits, -1 when a difference does not fit 32 bits signed, -2 when
 * `cap` is too small. */
int64_t rg_seg_bits(const int32_t *x, size_t T, uint8_t *bits, size_t cap, uint32_t *row_end)
{
  size_t n = 0;
  uint32_t last = 0;
  for (size_t t = 0; t < T; t++)
  {
    const uint32_t u = (uint32_t)x[t];
    const int64_t v = (int64_t)u - (int64_t)last;
    uint8_t cw[65];
    unsigned k;
    last = u;
    if (v < INT32_MIN || v > INT32_MAX)
      return -1;
    k = codeword(v, cw);
    if (n + k > cap)
      return -2;
    memcpy(bits + n, cw, k);
    n += k;
    if (row_end != NULL)
      row_end[t] = (uint32_t)n;
  }
  return (int64_t)n;
}

/* The coder on n binary symbols (one per byte).  Records the stream and its emit events (see rg_sink), the model at the
 * start of every word of 32 symbols -- word_tot = cum[0], word_f2 = the count of the less probable symbol, [ceil(n / 32)]
 * --, the symbols at whose update the two exchanged their indices (swap_sym) or the counts were halved (halve_sym).
 * counts[0..3] <- events, swaps, halvings, 0.  Returns the stream's bits, or -1 when a buffer was too small. */
int64_t rg_replay(const uint8_t *seg, size_t n, int adaptive, uint8_t *out_bits, size_t out_cap, uint32_t *ev_pos, uint32_t *ev_pend, uint32_t *ev_sym,
                  uint8_t *ev_bit, size_t ev_cap, uint32_t *word_tot, uint32_t *word_f2, uint32_t *swap_sym, size_t swap_cap, uint32_t *halve_sym, size_t halve_cap,
                  uint64_t *counts)
{
  rg_model_t m;
  rg_coder_t e = {0, 0xFFFFu, 0};
  rg_sink_t s;
  size_t swaps = 0, halvings = 0;
  memset(&s, 0, sizeof s);
  s.bits = out_bits;
  s.cap = out_cap;
  s.ev_pos = ev_pos;
  s.ev_pend = ev_pend;
  s.ev_sym = ev_sym;
  s.ev_bit = ev_bit;
  s.ev_cap = ev_cap;
  model_init(&m);
  for (size_t i = 0; i < n; i++)
  {
    if ((i & 31u) == 0 && word_tot != NULL)
    {
      word_tot[i >> 5] = m.cum[0];
      word_f2[i >> 5] = m.freq[2];
    }
    const unsigned idx = m.sym2idx[seg[i] & 1u];
    s.sym = i;
    encode_symbol(&e, &m, idx, &s);
    if (adaptive)
    {
      const int what = model_update(&m, idx);
      if (what & 1)
      {
        if (halve_sym != NULL && halvings < halve_cap)
          halve_sym[halvings] = (uint32_t)i;
        halvings++;
      }
      if (what & 2)
      {
        if (swap_sym != NULL && swaps < swap_cap)
          swap_sym[swaps] = (uint32_t)i;
        swaps++;
      }
    }
  }
  s.sym = n;
  encode_symbol(&e, &m, 3, &s); /* bac.c:163 */
  e.pending++;                  /* :143 */
  emit(&e, &s, e.start < RG_QUARTER ? 0 : 1);
  if (counts != NULL)
  {
    counts[0] = s.nev;
    counts[1] = swaps;
    counts[2] = halvings;
    counts[3] = 0;
  }
  if (s.overflow || (ev_pos != NULL && s.nev > ev_cap))
    return -1;
  return (int64_t)s.nbits;
}

/* The steerer, adaptive model.  out[0 .. n_head) <- head (coded as it is: it sets the model and the interval); then n_steer
 * samples whose seg bits are chosen one by one: the bit whose sub-interval still straddles the half point -- nothing gets
 * out, the owed bits grow -- until wanted[j] bits are owed; then, as soon as the other bit's sub-interval lies on the
 * wanted side of the half point (up != 0: above, the run ends in a carry; else below), that bit, and j moves on (cyclic).
 * The chosen bits are read as signed exp-Golomb codewords (the code is complete: any bit string parses); a zero prefix is
 * ended by force at maxprefix zeros, and the last bit of a codeword -- the sign -- is forced while the series is outside
 * [lo, hi].  Returns 0, or -1 when a sample leaves [0, 2^31). */
int rg_steer(const int32_t *head, size_t n_head, size_t n_steer, unsigned maxprefix, const uint32_t *wanted, size_t n_wanted, int up, int64_t lo, int64_t hi,
             int32_t *out)
{
  rg_model_t m;
  rg_coder_t e = {0, 0xFFFFu, 0};
  int64_t x = 0;
  size_t j = 0;
  model_init(&m);
  for (size_t t = 0; t < n_head; t++)
  {
    uint8_t bits[65];
    const int64_t v = (int64_t)(uint32_t)head[t] - x;
    unsigned n;
    if (v < INT32_MIN || v > INT32_MAX)
      return -1;
    n = codeword(v, bits);
    for (unsigned i = 0; i < n; i++)
    {
      const unsigned idx = m.sym2idx[bits[i]];
      encode_symbol(&e, &m, idx, NULL);
      model_update(&m, idx);
    }
    out[t] = head[t];
    x = (int64_t)(uint32_t)head[t];
  }
  for (size_t t = 0; t < n_steer; t++)
  {
    unsigned zeros = 0, left = 0;
    uint64_t w = 0;
    int in_prefix = 1;
    for (;;)
    {
      int forced = -1;
      unsigned bit;
      if (in_prefix && zeros >= maxprefix)
        forced = 1;
      else if (!in_prefix && left == 1)
      {
        /* the sign: w even <=> a positive difference (seg.c:25-28) */
        if (x > hi)
          forced = 1;
        else if (x < lo)
          forced = 0;
      }
      if (forced >= 0)
        bit = (unsigned)forced;
      else
      {
        uint32_t s1, e1, s2, e2;
        unsigned idx = 0;
        const uint32_t want = n_wanted != 0 ? wanted[j % n_wanted] : 0xFFFFFFFFu;
        narrow(&e, &m, 1, &s1, &e1);
        narrow(&e, &m, 2, &s2, &e2);
        {
          const int straddle1 = s1 <= e1 && s1 < RG_HALF && e1 >= RG_HALF, straddle2 = s2 <= e2 && s2 < RG_HALF && e2 >= RG_HALF;
          const int side1 = s1 <= e1 && (up ? s1 >= RG_HALF : e1 < RG_HALF), side2 = s2 <= e2 && (up ? s2 >= RG_HALF : e2 < RG_HALF);
          if (e.pending >= want && (side1 || side2))
          {
            idx = side1 ? 1 : 2;
            j++;
          }
          else if (straddle1 || straddle2)
            idx = straddle1 ? 1 : 2;
          else
            idx = side1 ? 1 : side2 ? 2 : 1;
        }
        bit = m.idx2sym[idx];
      }
      {
        const unsigned idx = m.sym2idx[bit];
        encode_symbol(&e, &m, idx, NULL);
        model_update(&m, idx);
      }
      if (in_prefix)
      {
        if (bit == 0)
          zeros++;
        else
        {
          in_prefix = 0;
          w = 1;
          left = zeros;
          if (left == 0)
            break;
        }
      }
      else
      {
        w = (w << 1) | bit;
        if (--left == 0)
          break;
      }
    }
    {
      const uint64_t cn = w - 1;
      int64_t v = (int64_t)((cn + 1) / 2);
      if ((cn & 1u) == 0)
        v = -v;
      x += v;
      if (x < 0 || x > INT32_MAX)
        return -1;
      out[n_head + t] = (int32_t)x;
    }
  }
  return 0;
}
