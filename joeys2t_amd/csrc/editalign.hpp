// The ALIGNMENT behind the unit-cost Levenshtein distance of two rows of int64 ids, computed by ONE wave (EXTENSION; the reference
// has no alignment on the device): which labels of the PIVOT row `a` are matched by the other row `b`.  confidence.hip calls it; the
// table, the back-trace and its tie rule are stated in the header above js2t_nbest_confidence.  It is the sibling of editdist.hpp's
// wave_edit_distance: the two share the walk of the table (edit_walk_tiles, where a tile's anti-diagonals are described) and the helpers.
//
// Forward pass.  The roles are not symmetric, so the orientation is fixed: the other row b lies across the lanes, the pivot runs down
// the rows; at step t lane c owns cell (x, y) = (t - c, k0 + c + 1).  The walk runs with CODES: every cell additionally decides
// which of the header's four cases the back-trace takes there - that depends on its three neighbours and the two symbols only - as
// a 2-bit code:
//     0 match (go to x-1, y-1, pivot position x-1 is matched)   1 substitution (x-1, y-1)   2 pivot label unmatched (x-1, y)
//     3 (x, y-1)
// A lane packs the codes of 16 consecutive rows of its column into one word and stores it at
//     codes[(tile * ceil(m / 16) + (x - 1) / 16) * 64 + lane]
// (a vector store; m = the pivot's trimmed length), so the pair's region holds align_code_words(longest row) words.  A table of
// one tile (k <= 64) and at most ALIGN_LDS_BLKS blocks of 16 rows (m <= 256) - every pair of the lists a beam search returns for
// an utterance of a few seconds - keeps its codes in the wave's LDS instead, under the same index: the boundary column, which only a
// second tile would read, is not written then (the walk runs without BND_ALWAYS), and its 4 KB hold the 16 x 64 words.
//
// Back-trace.  Behind a fence (codes in global memory only) all lanes walk the codes back from (m, k) in lockstep (every bound is wave-uniform; one word is
// loaded per step, the same for every lane) until a border of the table is reached: along x = 0 and y = 0 nothing is matched.  Lane w
// keeps word w of the result: bit (l & 31) of word l / 32 is set when pivot position l is matched.
//
// Short cuts.  The common SUFFIX of the two rows is trimmed and marked matched: that never changes the pivot's flags.  The common
// PREFIX is NOT trimmed: with a = [0, 0], b = [0] the rule gives [0, 1], a trimmed prefix would give [1, 0].
//
// Ids are compared as full 64-bit values, no id is a sentinel, and only a[0 .. m-1] and b[0 .. k-1] are read.
#pragma once
#include "editdist.hpp"

constexpr int ALIGN_MASK_WORDS = 64;  // one word per lane
constexpr int ALIGN_LDS_BLKS = EDIT_LDS_PER_WAVE / (64 * 4);  // blocks of 16 rows x 64 lanes whose code words the wave's LDS holds
static_assert(JS2T_EDIT_MAX_LEN <= ALIGN_MASK_WORDS * 32, "a lane per word of the match mask");

// words of the match mask of a pivot of at most L labels, and of the code region of a pair of rows of at most L labels
__host__ __device__ __forceinline__ int64_t align_mask_words(int64_t L) { return (L + 31) / 32; }
__host__ __device__ __forceinline__ int64_t align_code_words(int64_t L) { return ((L + 63) / 64) * ((L + 15) / 16) * 64; }

// bits lo .. hi-1 of the mask (lo <= hi), the part that falls into word `w`
__device__ __forceinline__ uint32_t align_range_bits(int w, int lo, int hi) {
  const int b0 = lo - w * 32 > 0 ? lo - w * 32 : 0, b1 = hi - w * 32 < 32 ? hi - w * 32 : 32;
  if (b0 >= b1) return 0u;
  const uint32_t upto = b1 == 32 ? 0xFFFFFFFFu : (1u << b1) - 1u;
  return upto & ~((1u << b0) - 1u);  // (b0 < 32 here)
}

// Every lane of the wave calls it with the same arguments (0 <= m, k <= JS2T_EDIT_MAX_LEN) and gets ITS word of the match mask of
// the pivot a (lane w: positions 32 w .. 32 w + 31; 0 behind m).  bnd: EDIT_CELLS cells of LDS, 4-byte aligned, that no other wave touches; codes:
// align_code_words(max(m, k)) words of global memory that no other wave touches (contents on entry do not matter).
__device__ __forceinline__ uint32_t wave_edit_align(const int64_t* a, int m, const int64_t* b, int k, uint16_t* bnd, uint32_t* codes) {
  const int lane = threadIdx.x & 63;
  if (m == 0 || k == 0) return 0u;
  const int full = m;
  const int suf = edit_common(a + m - 1, b + k - 1, m < k ? m : k, -1, lane);
  m -= suf, k -= suf;
  uint32_t mask = align_range_bits(lane, m, full);  // the common suffix is matched
  if (m == 0 || k == 0) return mask;
  const int xblks = (m + 15) >> 4;
  const bool in_lds = k <= 64 && xblks <= ALIGN_LDS_BLKS;  // (wave-uniform) the codes stay in the wave's LDS
  uint32_t* lcodes = reinterpret_cast<uint32_t*>(bnd);
  edit_walk_tiles<true, false>(a, m, b, k, bnd, codes, in_lds, lane);  // the pivot down the rows, b across the lanes
#ifdef JS2T_ALIGN_SKIP_TRACE  // timing builds of tools/confidence_bench.py only: the forward pass and its codes, no back-trace (wrong votes)
  return mask;
#endif
  if (!in_lds) __threadfence();  // the codes other lanes stored are read below
  const volatile uint32_t* rd = codes;
  int x = m, y = k;
  while (x > 0 && y > 0) {  // (wave-uniform)
    const uint32_t w = in_lds ? lcodes[((x - 1) >> 4) * 64 + (y - 1)] : rd[((int64_t)((y - 1) >> 6) * xblks + ((x - 1) >> 4)) * 64 + ((y - 1) & 63)];
    const uint32_t code = (w >> (((x - 1) & 15) * 2)) & 3u;
    if (code == 0u && ((x - 1) >> 5) == lane) mask |= 1u << ((x - 1) & 31);
    x -= code != 3u ? 1 : 0;
    y -= code != 2u ? 1 : 0;
  }
  return mask;
}
