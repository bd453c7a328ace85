// record_common.h -- what the two record formatters (sam.hip, bam.hip) share: a record is composed in LDS by a GROUP of W lanes of one
// wave (W = 64: one record per wave, sam.hip; W = 16: four records per wave, bam.hip) whose control flow is uniform within the group.
//   group_sync, group_sum<W>                  the wave helpers
//   ByteOut<EMIT, W>                          where a record's bytes go: bounded LDS stores, compiled out when !EMIT
//   cigar_sums<W>, sequence_of, md_walk       reference_cigar_length, the upper_bound over sequence_index, generate_md_string
#pragma once
#include "common.h"

namespace nvbio_amd {

__device__ __forceinline__ void wave_sync()
{
    // LDS operations of one wave execute in order; the fences keep the compiler from moving accesses of other lanes' bytes across this point
    __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
}
// the sum of v over the W lanes of a group (W consecutive lanes, W a power of two up to 64); the group's lanes are all active
template <uint32_t W>
__device__ __forceinline__ uint32_t group_sum(uint32_t v)
{
    for (int o = (int)W / 2; o; o >>= 1) v += __shfl_xor( v, o, 64 );
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(const uint32_t v) { return group_sum<64u>( v ); }
__device__ __forceinline__ uint32_t digits_of(const uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u :
           v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint8_t dna_char(const uint32_t s) { return s == 0u ? 'A' : s == 1u ? 'C' : s == 2u ? 'G' : s == 3u ? 'T' : 'N'; }   // dna.h:27-34

// where a record's bytes go: `buf` is the group's LDS (EMIT) and `at` the next byte; every store is bounded by `cap`.  The scalar
// fields are stored by lane 0 of the group, the striped ones by every lane.
template <bool EMIT, uint32_t W = 64u>
struct ByteOut
{
    uint8_t* buf;
    uint32_t cap, at, lane;
    __device__ __forceinline__ void store(const uint32_t p, const uint8_t c) const { if (EMIT && p < cap) buf[p] = c; }
    __device__ __forceinline__ void put(const uint8_t c) { if (lane == 0u) store( at, c ); ++at; }
    __device__ __forceinline__ void digits_at(const uint32_t p, uint32_t v, const uint32_t d) const           // the d digits of v, ending at p + d - 1
    {
        for (uint32_t k = d; k-- > 0u;) { store( p + k, (uint8_t)('0' + v % 10u) ); v /= 10u; }
    }
    __device__ __forceinline__ void put_uint(const uint32_t v)
    {
        const uint32_t d = digits_of( v );
        if (EMIT && lane == 0u) digits_at( at, v, d );
        at += d;
    }
    __device__ __forceinline__ void put_int(const int32_t v)                                                    // itoa, output_sam.cpp:76-115
    {
        if (v < 0) { put( '-' ); put_uint( 0u - (uint32_t)v ); } else put_uint( (uint32_t)v );
    }
    __device__ __forceinline__ void put_str(const char* s) { for (; *s; ++s) put( (uint8_t)*s ); }
    __device__ __forceinline__ void put_bytes(const uint8_t* src, const uint32_t n)                            // striped
    {
        if (EMIT) for (uint32_t k = lane; k < n; k += W) store( at + k, src[k] );
        at += n;
    }
};

// reference_cigar_length and the read length of a CIGAR (elements as the tracebacks write them: len << 2 | op, ops M I D S), and the width of
// its text; group-wide
template <uint32_t W = 64u>
__device__ __forceinline__ void cigar_sums(const uint16_t* cig, const uint32_t clen, const uint32_t lane, uint32_t* read_sum, uint32_t* ref_sum,
                                           uint32_t* text)
{
    uint32_t rs = 0u, fs = 0u, ts = 0u;
    for (uint32_t e = lane; e < clen; e += W)
    {
        const uint32_t el = cig[e], l = el >> 2, t = el & 3u;
        if (t != 2u) rs += l;
        if (t == 0u || t == 2u) fs += l;
        ts += digits_of( l ) + 1u;
    }
    *read_sum = group_sum<W>( rs ); *ref_sum = group_sum<W>( fs ); *text = group_sum<W>( ts );
}

// upper_bound( sequence_index, sequence_index + n_seqs, pos ) - 1 (output_sam.cpp:353-356)
__device__ __forceinline__ uint32_t sequence_of(const nvbio_sam_refs& refs, const uint32_t pos)
{
    uint32_t lo = 0u, hi = refs.n_seqs;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (refs.sequence_index_dev[mid] <= pos) lo = mid + 1u; else hi = mid; }
    return lo ? lo - 1u : 0u;
}

// generate_md_string (output_sam.cpp:216-289, output_bam.cpp:140-213) over the staged stream m[0, n): the MD text goes to `o`, the counts
// to mm / gapo / gape.  A byte past the stream reads as 0.  Match tokens that follow each other are summed in 32 bits (the reference sums
// them in a uint8).
template <class Out>
__device__ __forceinline__ void md_walk(const uint8_t* m, const uint32_t n, Out& o, int32_t* mm, int32_t* gapo, int32_t* gape)
{
    *mm = *gapo = *gape = 0;
    if (n <= 2u) return;
    auto B = [&](const uint32_t i) -> uint32_t { return i < n ? m[i] : 0u; };
    uint32_t i = 2u;
    do
    {
        const uint32_t op = B( i++ );
        if (op == 0u)
        {
            uint32_t l = B( i++ );
            while (i < n && m[i] == 0u) { l += B( i + 1u ); i += 2u; }
            o.put_uint( l );
        }
        else if (op == 1u) { o.put( dna_char( B( i++ ) ) ); ++*mm; }
        else if (op == 2u) { const uint32_t l = B( i++ ); i += l; ++*gapo; *gape += (int32_t)l - 1; }
        else if (op == 3u)
        {
            const uint32_t l = B( i++ );
            o.put( '^' );
            for (uint32_t k = 0; k < l; ++k) o.put( dna_char( B( i++ ) ) );
            o.put( '0' );
            ++*gapo; *gape += (int32_t)l - 1;
        }
    } while (i < n);
}

} // namespace nvbio_amd
