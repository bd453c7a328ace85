// bitplanes.h -- bit planes of packed reads and text windows for the ungapped shortcuts (band31_ungapped_inl.h, band31_chances.hip,
// gotoh_full.hip, gotoh_traceback.hip): bit i of (lo, hi, n) = low bit, high bit, "is N" of pattern row i; bit k of (tlo, thi) = the two
// bits of window symbol k.  Built a packed word at a time: bit-reverse the big-endian word so that symbol 0 sits lowest,
// squeeze every BITS-th bit together (3-4 shift/mask steps), drop the 8 / 16 plane bits at their storage offset, then
// shift the planes so that bit 0 is row 0 (reversed reads: mirror first).  Every word is loaded unconditionally (index
// clamped into the string, so always valid): no branches between the loads, they all issue back to back; plane bits
// outside the pattern / window are garbage and must be masked by the caller.
#pragma once
#include "common.h"

namespace nvbio_amd {

constexpr uint32_t PLANE_MAX_READ = 161u;                        // 3 x 64 bits hold 161 symbols at any storage offset

template <int RBITS> struct ReadWords { static constexpr int N = (161 + 15) * RBITS / 32 + 2; uint32_t w[N]; };
// (the loaders and converters of the packed text words, 13 of them or 14 -- one word more: 209 window symbols at any storage offset --,
// take any struct with that many words w[]: a job keeps them in the TextUnits below, which holds the text's bit planes if its batch carries them)

template <int RBITS>
__device__ __forceinline__ void load_read_words(const void* reads, const uint32_t first, const uint32_t M, ReadWords<RBITS>& out)
{
    constexpr uint32_t RPW = 32u / RBITS;
    const uint32_t* __restrict__ rwords = (const uint32_t*)reads;
    const uint32_t rw0 = (first & ~(RPW - 1u)) / RPW, rw_last = (first + M - 1u) / RPW;
    #pragma unroll
    for (int j = 0; j < ReadWords<RBITS>::N; ++j) { const uint32_t widx = rw0 + (uint32_t)j; out.w[j] = rwords[widx < rw_last ? widx : rw_last]; }
}

// T = number of window symbols that will be looked at (<= 16 WORDS - 15: 13 words hold 192 + 15 - offset, 14 words 209)
template <int WORDS, typename W>
__device__ __forceinline__ void load_text_words(const void* text, const uint32_t tb, const uint32_t T, W& out)
{
    const uint32_t* __restrict__ twords = (const uint32_t*)text;
    const uint32_t tw0 = (tb & ~15u) >> 4, tw_last = (tb + T - 1u) >> 4;
    #pragma unroll
    for (int j = 0; j < WORDS; ++j) { const uint32_t widx = tw0 + (uint32_t)j; out.w[j] = twords[widx < tw_last ? widx : tw_last]; }
}

__device__ __forceinline__ void shr192(uint64_t (&v)[3], const uint32_t sh)
{
    const uint32_t ws = sh >> 6, bs = sh & 63u;
    uint64_t x[5] = { v[0], v[1], v[2], 0ull, 0ull };
    uint64_t y[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = ws == 0u ? x[k] : (ws == 1u ? x[k + 1 < 5 ? k + 1 : 4] : (ws == 2u ? (k + 2 < 5 ? x[k + 2] : 0ull) : 0ull));
    #pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = bs ? ((y[k] >> bs) | (y[k + 1] << (64u - bs))) : y[k];
}
__device__ __forceinline__ void mirror192(uint64_t (&v)[3])
{
    const uint64_t a = __brevll( v[2] ), c = __brevll( v[0] );
    v[1] = __brevll( v[1] ); v[0] = a; v[2] = c;
}

// every 2nd bit of w (positions 0,2,..,30) squeezed into 16 bits
__device__ __forceinline__ uint32_t squeeze2(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u; x = (x | (x >> 2)) & 0x0F0F0F0Fu; x = (x | (x >> 4)) & 0x00FF00FFu; x = (x | (x >> 8)) & 0xFFFFu;
    return x;
}
// every 4th bit of w (positions 0,4,..,28) squeezed into 8 bits
__device__ __forceinline__ uint32_t squeeze4(uint32_t x)
{
    x &= 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u; x = (x | (x >> 6)) & 0x000F000Fu; x = (x | (x >> 12)) & 0xFFu;
    return x;
}

template <int RBITS>
__device__ __forceinline__ void read_planes192(const ReadWords<RBITS>& rw, const uint32_t first, const uint32_t M, const bool rev, const bool comp,
                                               uint64_t (&rlo)[3], uint64_t (&rhi)[3], uint64_t (&rn)[3])
{
    constexpr uint32_t RPW = 32u / RBITS;
    const uint32_t roff = first & (RPW - 1u);
    #pragma unroll
    for (int k = 0; k < 3; ++k) { rlo[k] = 0; rhi[k] = 0; rn[k] = 0; }
    #pragma unroll
    for (int j = 0; j < ReadWords<RBITS>::N; ++j)
    {
        // (the array covers 161 symbols at any offset; a wave of 150-symbol reads skips the words past their ends)
        if (!__any( (uint32_t)j * RPW < roff + M )) continue;
        const uint32_t w = __brev( rw.w[j] );
        uint32_t lo, hi, nn;
        if (RBITS == 4)
        {
            // after the reversal symbol k holds value bits (b3,b2,b1,b0) at bit positions (4k, 4k+1, 4k+2, 4k+3)
            lo = squeeze4( w >> 3 ); hi = squeeze4( w >> 2 ); nn = squeeze4( (w >> 1) | w );
        }
        else { lo = squeeze2( w >> 1 ); hi = squeeze2( w ); nn = 0; }
        const int bitpos = j * (int)RPW;                         // compile-time: no dynamic plane index
        if (bitpos < 192)
        {
            rlo[bitpos >> 6] |= (uint64_t)lo << (bitpos & 63);
            rhi[bitpos >> 6] |= (uint64_t)hi << (bitpos & 63);
            rn [bitpos >> 6] |= (uint64_t)nn << (bitpos & 63);
        }
    }
    // bit p of the planes = storage symbol (first - roff) + p.  Forward: row i = p - roff.  Reversed: row i = roff + M-1 - p.
    if (rev)
    {
        mirror192( rlo ); mirror192( rhi ); mirror192( rn );    // bit r now = storage symbol base + 191 - r
        const uint32_t sh = 192u - roff - M;                     // row i = bit i + sh
        shr192( rlo, sh ); shr192( rhi, sh ); shr192( rn, sh );
    }
    else { shr192( rlo, roff ); shr192( rhi, roff ); shr192( rn, roff ); }
    if (comp)                                                    // 3 - q for q < 4: flip both bits of the non-N rows
    {
        #pragma unroll
        for (int k = 0; k < 3; ++k) { rlo[k] ^= ~rn[k]; rhi[k] ^= ~rn[k]; }
    }
}

// rows 64 k .. 64 k + 63 of a read's planes (read_planes192; M rows in all) as 32-bit words 2 k, 2 k + 1: bit j of word w of (pl, ph, pn, pm)
// = row 32 w + j (its symbol's low / high bit, N, a row of the read at all; pn holds no bit past the read's end).  (One k per call: PlaneWords::set
// fills its text words between them, and with all three k in front of those the gap chance's kernels compile to other code.)
__device__ __forceinline__ void pattern_plane_words(const int k, const uint64_t (&rlo)[3], const uint64_t (&rhi)[3], const uint64_t (&rn)[3], const uint32_t M,
                                                    uint32_t (&pl)[6], uint32_t (&ph)[6], uint32_t (&pn)[6], uint32_t (&pm)[6])
{
    const int32_t left = (int32_t)M - 64 * k;
    const uint64_t mask = left >= 64 ? ~0ull : (left > 0 ? ((1ull << left) - 1ull) : 0ull);
    pl[2*k] = (uint32_t)rlo[k]; pl[2*k+1] = (uint32_t)(rlo[k] >> 32);
    ph[2*k] = (uint32_t)rhi[k]; ph[2*k+1] = (uint32_t)(rhi[k] >> 32);
    pm[2*k] = (uint32_t)mask;   pm[2*k+1] = (uint32_t)(mask >> 32);
    pn[2*k] = (uint32_t)rn[k] & pm[2*k]; pn[2*k+1] = (uint32_t)(rn[k] >> 32) & pm[2*k+1];
}

// 16 WORDS plane bits (13 packed words: 208, 14: 224), shifted so that bit 0 = window symbol 0; the top word holds the remainder
template <int WORDS, typename W>
__device__ __forceinline__ void text_planes_words(const W& tw, const uint32_t tb, uint64_t (&tlo)[4], uint64_t (&thi)[4])
{
    static_assert( WORDS <= 16, "four 64-bit plane words" );
    #pragma unroll
    for (int k = 0; k < 4; ++k) { tlo[k] = 0; thi[k] = 0; }
    #pragma unroll
    for (int j = 0; j < WORDS; ++j)
    {
        const uint32_t w = __brev( tw.w[j] );
        const uint32_t lo = squeeze2( w >> 1 ), hi = squeeze2( w );
        const int bitpos = j * 16;
        tlo[bitpos >> 6] |= (uint64_t)lo << (bitpos & 63);
        thi[bitpos >> 6] |= (uint64_t)hi << (bitpos & 63);
    }
    const uint32_t toff = tb & 15u;
    if (toff)
    {
        #pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            tlo[k] = (tlo[k] >> toff) | (tlo[k + 1] << (64u - toff));
            thi[k] = (thi[k] >> toff) | (thi[k + 1] << (64u - toff));
        }
        tlo[3] >>= toff; thi[3] >>= toff;
    }
}

// ---- the text kept as bit planes (nvbio_text_planes_build, fm_build.hip) ---------------------------------------------------------
// A unit is 16 bytes, (lo64, hi64) of 64 consecutive text symbols: bit j of lo64 / hi64 = the low / high bit of symbol 64 u + j.  Line L
// (128 bytes, 128-byte aligned) holds units 4 L .. 4 L + 7, i.e. symbols 256 L .. 256 L + 511: consecutive lines overlap by half, the
// array has ((n + 255) >> 8) + 1 lines, and every bit at or beyond symbol n is zero.
constexpr uint32_t TEXT_PLANE_LINE_BYTES = 128u;
inline __host__ __device__ uint64_t text_plane_lines(const uint32_t n) { return (((uint64_t)n + 255u) >> 8) + 1u; }

// The planes of the UNITS * 64 - 63 or more symbols from tb on, in the form text_planes_words returns: UNITS aligned 16-byte
// loads from ONE line (load_text_units: issued with the read's loads), then a funnel shift by tb & 63 on 32-bit halves (text_planes_units).  Bits past the text's end are zero, bits past the window's end are
// the text's next symbols (the caller masks them, as with the packed words).
// Extent: the window begins in line tb >> 8 at unit u0 = (tb & 255) >> 6 <= 3 with shift s = tb & 63 <= 63, so E symbols end in unit
// u0 + ((s + E - 1) >> 6).  A single job looks at E <= 192 symbols: s + E - 1 <= 254, 4 units, last index <= 6.  A gap-chance pair looks
// at E <= 161 + 31 + 5 = 197: s + E - 1 <= 259, 5 units, last index <= 7 -- always inside the line's 8 units.
// w[4 j .. 4 j + 3] = unit j as loaded: lo64's two words, hi64's two words (or, in a batch without planes, the 13 / 14 packed words)
template <int UNITS> struct TextUnits { uint32_t w[4 * UNITS]; };

// (units FROM .. TO - 1 of the window: a kernel that has no registers to spare for all of them beside the read's words in flight takes the
// last one -- a hit in the line the others brought -- once the read's words are consumed)
template <int UNITS, int FROM = 0, int TO = UNITS>
__device__ __forceinline__ void load_text_units(const void* planes, const uint32_t tb, TextUnits<UNITS>& out)
{
    static_assert( UNITS == 4 || UNITS == 5, "4 units hold 192 symbols at any shift, 5 units hold 197" );
    static_assert( 3 + UNITS - 1 <= 7, "the last unit of a window lies in the line its first unit lies in" );
    typedef uint32_t unit_t __attribute__((ext_vector_type(4)));  // one global_load_dwordx4
    const unit_t* __restrict__ p = (const unit_t*)planes + ((size_t)(tb >> 8) * 8u + ((tb & 255u) >> 6));
    #pragma unroll
    for (int j = FROM; j < TO; ++j) { const unit_t v = p[j]; out.w[4*j] = v.x; out.w[4*j+1] = v.y; out.w[4*j+2] = v.z; out.w[4*j+3] = v.w; }
}

template <int UNITS>
__device__ __forceinline__ void text_planes_units(const TextUnits<UNITS>& tu, const uint32_t tb, uint64_t (&tlo)[4], uint64_t (&thi)[4])
{
    const uint32_t s = tb & 63u;
    const uint32_t up = s >= 32u ? 0xFFFFFFFFu : 0u;             // v_alignbit takes s & 31: the other 32 by choosing the words (one v_bfi
                                                                 // each; written as a mask so that it stays a choice between registers)
    // word i of the lo / hi plane as loaded, zeros past the last unit
    auto lo = [&](const int i) { return i < 2 * UNITS ? tu.w[4 * (i >> 1) + (i & 1)] : 0u; };
    auto hi = [&](const int i) { return i < 2 * UNITS ? tu.w[4 * (i >> 1) + 2 + (i & 1)] : 0u; };
    uint32_t a[9], c[9];
    #pragma unroll
    for (int i = 0; i < 9; ++i) { a[i] = (lo( i + 1 ) & up) | (lo( i ) & ~up); c[i] = (hi( i + 1 ) & up) | (hi( i ) & ~up); }
    #pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        tlo[k] = (uint64_t)__builtin_amdgcn_alignbit( a[2*k+1], a[2*k], s ) | ((uint64_t)__builtin_amdgcn_alignbit( a[2*k+2], a[2*k+1], s ) << 32);
        thi[k] = (uint64_t)__builtin_amdgcn_alignbit( c[2*k+1], c[2*k], s ) | ((uint64_t)__builtin_amdgcn_alignbit( c[2*k+2], c[2*k+1], s ) << 32);
    }
}

// ---- the seed locus lines (nvbio_seed_locus_build, fm_index.hip) ------------------------------------------------------------------
// The text's bit planes once more, beside a uniqueness plane u for ONE seed length: u[x] = 1 only if text[x, x + len) occurs once in the
// text, its reverse complement nowhere, and the canonical table answers both of them from its rows (fm_canon_inl.h: seed_locus_kernel).
// A unit is 24 bytes, (lo64, hi64, u64) of 64 consecutive text symbols: lo64 / hi64 as in the planes above, bit j of u64 = u[64 unit + j].
// Line L (128 bytes, 128-byte aligned) holds units 2 L .. 2 L + 4, i.e. symbols 128 L .. 128 L + 319, then 8 zero bytes; the array has
// (n >> 7) + 1 lines and every bit at or beyond symbol n is zero.
// Extent: a read placed at text position P0 lies in line P0 >> 7 from symbol offset P0 & 127 <= 127 on, so a read of M symbols ends at or
// before offset 127 + M - 1 <= 319 for M <= 193: ONE line holds every seed window of the read.
constexpr uint32_t SEED_LOCUS_LINE_BYTES = 128u;
constexpr uint32_t SEED_LOCUS_UNITS      = 5u;                   // units of 64 symbols in a line
constexpr uint32_t SEED_LOCUS_MAX_READ   = 193u;
inline __host__ __device__ uint64_t seed_locus_lines(const uint32_t n) { return ((uint64_t)n >> 7) + 1u; }

// Of the read at `base`, the 32-bit word of each plane that holds symbol x (x >= base, x + len - 1 <= base + SEED_LOCUS_MAX_READ - 1) and the
// word behind it, and the word of u that holds u[x]: a window of len <= 32 symbols spans no more.  As 32-bit words a unit is
// (lo, lo', hi, hi', u, u'); the word behind a unit's second word is the first word of the next unit, 24 bytes on.
struct LocusWords { uint32_t lo0, lo1, hi0, hi1, u; };

__device__ __forceinline__ void load_locus_words(const void* __restrict__ lines, const uint32_t base, const uint32_t x, LocusWords& out)
{
    static_assert( 127u + SEED_LOCUS_MAX_READ - 1u <= 64u * SEED_LOCUS_UNITS - 1u, "the last symbol of a read lies in the line its first symbol lies in" );
    static_assert( 24u * SEED_LOCUS_UNITS <= SEED_LOCUS_LINE_BYTES, "a line holds its units" );
    const uint32_t line = base >> 7, off = x - (line << 7), unit = off >> 6, w = (off >> 5) & 1u;   // unit <= 4
    const uint32_t* __restrict__ p = (const uint32_t*)lines + ((size_t)line * 32u + 6u * unit);
    // (a window that crosses into the next unit has one: in the line's last unit the second word read is one the window does not reach)
    const uint32_t w1 = w ? (unit + 1u < SEED_LOCUS_UNITS ? 6u : 0u) : 1u;
    out.lo0 = p[w]; out.lo1 = p[w1]; out.hi0 = p[2u + w]; out.hi1 = p[2u + w1]; out.u = p[4u + w];
}

// does text[x, x + len) equal the len <= 32 symbols whose bit planes are (tlo, thi) (bit t: symbol t; bits from len on are ignored), with u[x] set?
__device__ __forceinline__ bool locus_answers(const LocusWords& lw, const uint32_t x, const uint32_t len, const uint32_t tlo, const uint32_t thi)
{
    const uint32_t s = x & 31u;
    const uint32_t lo = __builtin_amdgcn_alignbit( lw.lo1, lw.lo0, s ), hi = __builtin_amdgcn_alignbit( lw.hi1, lw.hi0, s );
    const uint32_t mask = len >= 32u ? 0xFFFFFFFFu : (1u << len) - 1u;
    return ((((lo ^ tlo) | (hi ^ thi)) & mask) == 0u) && ((lw.u >> s) & 1u);
}

} // namespace nvbio_amd
