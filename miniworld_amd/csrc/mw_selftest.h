// What mw_selftest_sincosf (mw_selftest.hip) sums on the device and the host tests sum from libm and the oracle
// (tests/hostcheck/mwhost.cpp): one definition of the hash and of the f64 input stream for both sides.
#pragma once
#include <stdint.h>
#include <string.h>
#include "mw_hd.h"

namespace mwcheck {

MW_HD uint64_t mix64(uint64_t z)         // splitmix64's finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MW_HD uint32_t float_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return x != x ? 0x7fc00000u : u; }     // NaN: canonical
MW_HD uint64_t double_bits(double x) { uint64_t u; memcpy(&u, &x, 8); return x != x ? 0x7ff8000000000000ull : u; }

// one evaluation of sinf / cosf at the float with bits x; summed per binade (sign | exponent, x >> 23) mod 2^64, so the
// order in which the lanes or threads add them does not matter
MW_HD uint64_t hash_sincosf(uint32_t x, float s, float c)
{
    return mix64(mix64(((uint64_t)x << 32 | float_bits(s)) + 0x9E3779B97F4A7C15ull) ^ float_bits(c));
}

MW_HD uint64_t hash_sincos(double x, double s, double c)
{
    return mix64(mix64(mix64(double_bits(x) + 0x9E3779B97F4A7C15ull) ^ double_bits(s)) ^ double_bits(c));
}

// the f64 headings' check stream: input i is a double with a uniform 52-bit mantissa, an exponent uniform over
// 2^-40 .. 2^19 and the sign of i's low bit, folded below 1e6 (mw::sincos_det's domain); its bin (0 .. 119) is
// sign * 60 + the exponent's index
MW_HD double heading_sample(uint64_t i, int &bin)
{
    const uint64_t z = mix64(i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull);
    const int e = (int)((z >> 52) % 60u) - 40;
    const uint64_t u = (i & 1u) << 63 | (uint64_t)(1023 + e) << 52 | (z & 0xFFFFFFFFFFFFFull);
    double x;
    memcpy(&x, &u, 8);
    if (x >= 1e6) x -= 524288.0;
    if (x <= -1e6) x += 524288.0;
    bin = (int)(i & 1u) * 60 + (e + 40);
    return x;
}

}  // namespace mwcheck
