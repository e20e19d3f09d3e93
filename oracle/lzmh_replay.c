/* lzmh_replay.c -- an instrumented replay of the reference's greedy LZMH parse and of its coder, behind
 * tests/lzmh_encoder_common.py.  TEST INFRASTRUCTURE ONLY (see dega_oracle.h).
 *
 * Written from the format and the behaviour that lzmh_oracle.c describes, without its 403-byte ring: with P bytes consumed,
 * look back at most min(P, 128) bytes and ahead at most min(274, min(n, max(P - 128, 0) + 403) - P) bytes; scan the offsets
 * upward and take a match that is LONGER than the best so far (so the nearest of equals stays); three bytes or more are
 * coded as a match, anything less as one literal through the frequency list.  An input of exactly 403 bytes gives nothing.
 * The replay writes the stream as well, and its caller hands a trace out only after that stream has been found to be
 * orc_lzmh_encode's, bit for bit: what the trace says about the steps is then what the oracle's parse did.
 *
 * One record of LZR_COLS int32 per step:
 *   0 position P   1 match length (0: a literal)   2 offset (0: a literal)
 *   3 code: 0..3 the k-th most recent offset | 4 a new offset | 5 a literal by its list position | 6 a raw literal
 *   4 offsets within reach whose three bytes equal the next three of the input (0 where fewer than 3 bytes may be matched)
 *   5 how often the best length improved during the scan
 *   6 the literal's byte   7 the list position it was found at (-1: not in the list)
 *   8 1 when it was not in the list and the list was full (the literal is dropped from the statistics)
 *   9 how many entries it moved towards the front
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define LZR_COLS 10
#define MAX_OFFSET 128
#define MAX_LENGTH 274
#define RING 403
#define LIST_LEN 48
#define TREE_LEN 19

typedef struct
{
  uint8_t *data;
  size_t cap, nbits;
  int overflow;
} sink_t;

static void put(sink_t *s, uint32_t v, unsigned k) /* low k bits of v, MSB first */
{
  while (k > 0)
  {
    k--;
    if (s->nbits / 8 >= s->cap)
    {
      s->overflow = 1;
      return;
    }
    if ((v >> k) & 1u)
      s->data[s->nbits >> 3] |= (uint8_t)(0x80u >> (s->nbits & 7));
    s->nbits++;
  }
}

static void put_list_code(sink_t *s, int p) /* 4 codes of 4 bits, 5 of 5, 4 of 6, 2 of 7, 4 of 8 */
{
  if (p >= 15)
    put(s, 0x83u - (unsigned)(p - 15), 8);
  else if (p >= 13)
    put(s, 0x43u - (unsigned)(p - 13), 7);
  else if (p >= 9)
    put(s, 0x25u - (unsigned)(p - 9), 6);
  else if (p >= 4)
    put(s, 0x17u - (unsigned)(p - 4), 5);
  else
    put(s, 0x0Fu - (unsigned)p, 4);
}

/* -> the number of steps, -1 when rec or stream is too small.  stream must come zeroed. */
int64_t lzr_replay(const uint8_t *text, size_t n, int32_t *rec, size_t max_steps, uint8_t *stream, size_t stream_cap, uint64_t *nbits)
{
  uint8_t sym[LIST_LEN];
  int count[LIST_LEN];
  int mru[4] = { 0, 0, 0, 0 };
  sink_t s = { stream, stream_cap, 0, 0 };
  size_t P = 0, steps = 0;
  memset(sym, 0, sizeof(sym));
  memset(count, 0, sizeof(count));
  *nbits = 0;
  if (n == RING)
    return 0;
  while (P < n)
  {
    const size_t maxoff = P < MAX_OFFSET ? P : MAX_OFFSET;
    size_t have = (P > MAX_OFFSET ? P - MAX_OFFSET : 0) + RING;
    size_t maxlen, o, best = 2, besto = 0;
    int32_t *r;
    int cand = 0, improved = 0;
    if (have > n)
      have = n;
    maxlen = have - P > MAX_LENGTH ? MAX_LENGTH : have - P;
    if (maxlen >= 3)
      for (o = 1; o <= maxoff; o++)
        cand += text[P - o] == text[P] && text[P - o + 1] == text[P + 1] && text[P - o + 2] == text[P + 2];
    for (o = 1; o <= maxoff && best < maxlen; o++)
      if (text[P - o] == text[P] && text[P - o + best] == text[P + best])
      {
        size_t l = 1;
        while (l < maxlen && text[P - o + l] == text[P + l])
          l++;
        if (l > best)
        {
          best = l;
          besto = o;
          improved++;
        }
      }
    if (steps >= max_steps)
      return -1;
    r = rec + LZR_COLS * steps++;
    memset(r, 0, LZR_COLS * sizeof(int32_t));
    r[0] = (int32_t)P;
    r[4] = cand;
    r[5] = improved;
    r[7] = -1;
    if (best >= 3)
    {
      int k;
      for (k = 0; k < 4 && mru[k] != (int)besto; k++)
        ;
      r[1] = (int32_t)best;
      r[2] = (int32_t)besto;
      r[3] = k;
      if (k == 0)
        put(&s, 0x06, 4);
      else if (k == 1)
        put(&s, 0x0E, 5);
      else if (k == 2)
        put(&s, 0x1E, 6);
      else if (k == 3)
        put(&s, 0x1F, 6);
      else
        put(&s, 0x100u | (unsigned)(besto - 1), 10);
      for (k = k < 3 ? k : 3; k > 0; k--) /* to the front; a new offset pushes the oldest out */
        mru[k] = mru[k - 1];
      mru[0] = (int)besto;
      if (best < 11)
        put(&s, (unsigned)(best - 3), 4);
      else if (best < 19)
        put(&s, 0x10u | (unsigned)(best - 11), 5);
      else
        put(&s, 0x300u | (unsigned)(best - 19), 10);
      P += best;
    }
    else
    {
      const uint8_t b = text[P++];
      int i = 0, found = -1;
      while (i < LIST_LEN && count[i] > 0 && sym[i] != b)
        i++;
      r[6] = b;
      if (i < LIST_LEN && count[i] > 0)
      {
        found = i;
        if (count[i] < 65535)
        {
          const int nc = count[i] + 1;
          while (i > 0 && nc > count[i - 1]) /* only the symbols move */
          {
            sym[i] = sym[i - 1];
            i--;
          }
          count[i] = nc;
          sym[i] = b;
        }
        r[9] = found - i;
      }
      else if (i < LIST_LEN)
      {
        sym[i] = b;
        count[i] = 1;
      }
      else
        r[8] = 1;
      r[7] = found;
      if (found >= 0 && found < TREE_LEN)
      {
        r[3] = 5;
        put_list_code(&s, found);
      }
      else
      {
        r[3] = 6;
        put(&s, b, 10);
      }
    }
    if (s.overflow)
      return -1;
  }
  *nbits = s.nbits;
  return (int64_t)steps;
}
