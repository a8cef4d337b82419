// forest_key.h — the order of the edges of `mash cluster -T` (cluster_forest.hip), as plain C++ that a device kernel, the emulator
// program and a stand-alone CPU check can include.
//
// THE ORDER.  Edge a ranks before edge b iff numer_a * denom_b > numer_b * denom_a in 64-bit integers (the fraction `mash triangle
// -E` prints in column 5, larger first); equal fractions, also under different denominators, by ascending row, then ascending column.
// denom == 0 (two empty sketches) implies numer == 0; such a pair is compared as 0/1, as topk.hip does: the bare products would tie
// it with everything.
//
// THE KEY.  key = floor(numer * 2^42 / denom), for denom < 2^21 (numer <= denom: the product is below 2^63).
// Lemma: for a/b > c/d with b, d < 2^21:  2^42 a/b - 2^42 c/d = 2^42 (ad - bc) / (bd) >= 2^42 / (bd) > 1, so the two floors differ
// and in that direction; equal fractions have equal quotients, hence equal keys.  The key's order IS the fraction's order -- which
// lets a component's best weight be found with one 64-bit atomicMax.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MG_FOREST_HD __host__ __device__ inline
#else
#define MG_FOREST_HD inline
#endif

namespace mg {

constexpr uint32_t FOREST_DENOM_LIMIT = 1u << 21;              // the key is exact for denominators below this

MG_FOREST_HD unsigned long long forest_key(uint32_t numer, uint32_t denom)
{
    return ((unsigned long long)numer << 42) / (denom ? denom : 1u);
}

// THE WEIGHT of an edge in a row's centrality score (`mash cluster -M`, cluster_medoid.hip): floor(numer * 2^32 / max(denom, 1)), at most
// 2^32 because numer <= denom; 0/0 counts as 0/1 as above.  A fixed point only so that fractions under different denominators can be
// summed in integers: fewer than 2^31 edges at a row keep the sum below 2^63.
MG_FOREST_HD unsigned long long medoid_weight(uint32_t numer, uint32_t denom)
{
    return ((unsigned long long)numer << 32) / (denom ? denom : 1u);
}

// the row pair as one word: ascending {row, col} is ascending rc
MG_FOREST_HD unsigned long long forest_rc(uint32_t row, uint32_t col) { return (unsigned long long)row << 32 | col; }

// a ranks strictly before b: the cross-multiplication itself, for every numer <= denom < 2^32
MG_FOREST_HD bool forest_before(uint32_t numer_a, uint32_t denom_a, unsigned long long rc_a, uint32_t numer_b, uint32_t denom_b, unsigned long long rc_b)
{
    const unsigned long long l = (unsigned long long)numer_a * (denom_b ? denom_b : 1u);
    const unsigned long long r = (unsigned long long)numer_b * (denom_a ? denom_a : 1u);
    return l > r || (l == r && rc_a < rc_b);
}

}  // namespace mg
