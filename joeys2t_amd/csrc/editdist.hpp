// Unit-cost Levenshtein distance of two rows of int64 ids, computed by ONE wave (EXTENSION; the reference has no edit distance on the
// device).  mbr.hip's two entry points call it; the semantics they give it are stated in the header.
//
// One row lies across the lanes, 64 columns per tile, every lane keeping its own symbol in registers - for the distance the shorter
// one; the other row runs down the rows of the table.  A tile is walked by anti-diagonals (edit_walk_tiles): at step t lane c owns cell (t - c, c).  `up` is the lane's own
// previous value, `left` the previous lane's value of step t - 1 (one shuffle per step), `diag` what that shuffle returned the step
// before.  The long row's symbols ride the same way: lane 0 takes symbol t from a 64-symbol register chunk (one coalesced load per
// 64 steps), every other lane takes its neighbour's.  A tile costs n_long + 64 steps.  A short row of more than 64 symbols runs tile
// after tile: lane 63 leaves the tile's right boundary column in LDS that belongs to the wave alone, lane 0 of the next tile reads
// it - behind the rows lane 63 overwrites in the same pass, so one column is enough.  No block barrier, no global workspace, no
// atomics.
//
// Short cuts, exact for Levenshtein: an empty row gives the other's length, and the common prefix and the common suffix of the two
// rows are trimmed before the table is walked (the hypotheses of one n-best list share most of their labels).
//
// Ids are compared as full 64-bit values, no id is a sentinel, and only a[0 .. na-1] and b[0 .. nb-1] are read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/joeys2t_hip.h"

// The boundary column holds one 16-bit cell per row of the table, row 0 included (a distance is at most the longer length, so 16
// bits hold it): EDIT_LDS_PER_WAVE bytes of LDS per wave, four waves per block = 16 KB, which leaves a CU room for ten blocks.
constexpr int EDIT_LDS_PER_WAVE = 4096;
static_assert(JS2T_EDIT_MAX_LEN == EDIT_LDS_PER_WAVE / 2 - 1, "the header's JS2T_EDIT_MAX_LEN is what the boundary column holds");
static_assert(JS2T_EDIT_MAX_LEN >= 1024 && JS2T_EDIT_MAX_LEN < 65536, "16-bit cells");
constexpr int EDIT_CELLS = JS2T_EDIT_MAX_LEN + 1;

__device__ __forceinline__ int64_t edit_shfl_up1(int64_t v) {
  const int lo = __shfl_up((int)(uint32_t)v, 1, 64), hi = __shfl_up((int)(v >> 32), 1, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t edit_read_lane(int64_t v, int src) {  // (src wave-uniform)
  const int lo = __shfl((int)(uint32_t)v, src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// the number of leading positions < m at which x[i * dir] == y[i * dir] (dir = 1: common prefix; dir = -1 from the last
// elements: common suffix), 64 positions per step
__device__ __forceinline__ int edit_common(const int64_t* x, const int64_t* y, int m, int dir, int lane) {
  int c = 0;
  while (c < m) {  // (wave-uniform: c and m are)
    const int i = c + lane;
    const bool ne = i < m && x[(int64_t)i * dir] != y[(int64_t)i * dir];
    const unsigned long long mask = __ballot(ne);
    if (mask) return c + __builtin_ctzll(mask);
    c = c + 64 < m ? c + 64 : m;
  }
  return c;
}

// The walk of one table, tile after tile - the one statement of it, for wave_edit_distance below and for editalign.hpp's
// wave_edit_align.  Every lane of the wave calls it with the same arguments: the row `down` (nd >= 1 symbols) runs down the rows of
// the table, `across` (nc >= 1) lies across the lanes; bnd as below.  Returns the lane's last cell: lane (nc - 1) & 63 holds
// D[nd][nc].  The two compile-time switches are all the two callers differ in here:
//   CODES: every cell also records which of the four cases of editalign.hpp the back-trace takes there, 16 rows of a column to a
//     word, in `codes` - or, with in_lds (wave-uniform), in bnd itself, which only a one-tile table may ask for;
//   BND_ALWAYS: lane 63 writes the boundary column in every tile; without it only where a next tile reads it (which leaves bnd to the
//     codes of a one-tile table).
template <bool CODES, bool BND_ALWAYS>
__device__ __forceinline__ int edit_walk_tiles(const int64_t* down, int nd, const int64_t* across, int nc, uint16_t* bnd, uint32_t* codes,
                                               bool in_lds, int lane) {
  const int xblks = (nd + 15) >> 4;
  uint32_t* lcodes = reinterpret_cast<uint32_t*>(bnd);
  int val = 0;
  for (int k0 = 0; k0 < nc; k0 += 64) {  // (every bound below is wave-uniform: all lanes reach every shuffle)
    const int cols = nc - k0 < 64 ? nc - k0 : 64;
    const bool col = lane < cols, more = k0 + 64 < nc;  // more: a next tile reads this one's boundary column
    const int64_t cs = col ? across[k0 + lane] : 0;
    uint32_t* tile = CODES ? codes + (int64_t)(k0 >> 6) * xblks * 64 : nullptr;
    val = k0 + lane + 1;  // row 0 of the table
    int diag = k0;        // (lane 0's: row 0 of the boundary column; every other lane's comes with the first shuffle)
    int64_t ds = 0, chunk = 0;
    uint32_t cw = 0;
    const int steps = nd + cols - 1;
    for (int t = 1; t <= steps; ++t) {
      if (((t - 1) & 63) == 0) chunk = t - 1 + lane < nd ? down[t - 1 + lane] : 0;
      int left = __shfl_up(val, 1, 64);
      ds = edit_shfl_up1(ds);
      const int64_t head = edit_read_lane(chunk, (t - 1) & 63);
      if (lane == 0) {
        ds = head;
        left = k0 ? (int)bnd[t < nd ? t : nd] : t;
      }
      const int x = t - lane;  // the row this lane is in
      if (col && x >= 1 && x <= nd) {
        const bool eq = ds == cs;
        const int sub = diag + (eq ? 0 : 1);
        uint32_t code = 0u;
        if (CODES) {  // the three neighbours apart: the code asks which of them the minimum came from
          const int del = val + 1, ins = left + 1;
          const int d = sub < del ? (sub < ins ? sub : ins) : (del < ins ? del : ins);
          code = (eq && d == diag) ? 0u : d == diag + 1 ? 1u : d == del ? 2u : 3u;  // the FIRST case that applies
          val = d;
        } else {
          const int ins = (val < left ? val : left) + 1;
          val = sub < ins ? sub : ins;
        }
        if (lane == 63 && (BND_ALWAYS || more)) bnd[x] = (uint16_t)val;
        if (CODES) {
          cw |= code << (((x - 1) & 15) * 2);
          if (((x - 1) & 15) == 15 || x == nd) {
            if (in_lds) lcodes[((x - 1) >> 4) * 64 + lane] = cw;
            else tile[(int64_t)((x - 1) >> 4) * 64 + lane] = cw;
            cw = 0;
          }
        }
      }
      diag = left;
    }
  }
  return val;
}

// Every lane of the wave calls it with the same arguments (0 <= na, nb <= JS2T_EDIT_MAX_LEN) and gets the distance; bnd: EDIT_CELLS
// cells of LDS that no other wave touches (contents on entry do not matter).
__device__ __forceinline__ int wave_edit_distance(const int64_t* a, int na, const int64_t* b, int nb, uint16_t* bnd) {
  const int lane = threadIdx.x & 63;
  if (na == 0 || nb == 0) return na + nb;
  const int pre = edit_common(a, b, na < nb ? na : nb, 1, lane);
  a += pre, b += pre, na -= pre, nb -= pre;
  const int suf = edit_common(a + na - 1, b + nb - 1, na < nb ? na : nb, -1, lane);
  na -= suf, nb -= suf;
  if (na == 0 || nb == 0) return na + nb;
  const int64_t* L = na >= nb ? a : b;  // down the rows
  const int64_t* S = na >= nb ? b : a;  // across the lanes: the shorter row
  const int nl = na >= nb ? na : nb, ns = na >= nb ? nb : na;
  const int val = edit_walk_tiles<false, true>(L, nl, S, ns, bnd, nullptr, false, lane);
  return __shfl(val, (ns - 1) & 63, 64);
}
