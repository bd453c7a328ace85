// byte_scan.h -- what the text parsers (fastq.hip, fasta.hip) share: a sequential machine over bytes run as a prefix scan.
// A byte is a FUNCTION over the machine's states, at most six of them, six 3-bit fields of one register: field s holds the state that
// state s goes to.  Functions compose associatively, (f then g)[s] = g[f[s]], so the state in front of every byte comes from a scan:
// 16 bytes per lane (one 16-byte load), lanes across the wave with cross-lane moves, waves through LDS, 4096-byte tiles through an
// array that ONE workgroup scans in a launch of its own.  No workgroup waits on another.
#pragma once
#include "common.h"

namespace nvbio_amd {

static constexpr uint32_t BS_TILE = 4096u;                                          // bytes per workgroup: 256 lanes x 16
static constexpr uint32_t BS_IDENTITY = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12) | (5u << 15);

// f, then g
__device__ __forceinline__ uint32_t bs_compose(const uint32_t f, const uint32_t g)
{
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t s = 0u; s < 18u; s += 3u) r |= ((g >> (3u * ((f >> s) & 7u))) & 7u) << s;
    return r;
}

// the 16 bytes of this lane: text[at, at + 16), the bytes of `pad` (one whose function is the identity) behind the text
__device__ __forceinline__ void bs_load16(const uint8_t* __restrict__ text, const uint32_t n, const uint64_t at, const uint32_t pad, uint32_t w[4])
{
    if (at + 16u <= n) { const uint4 v = *(const uint4*)(text + at); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; return; }
    w[0] = w[1] = w[2] = w[3] = pad;
    for (uint32_t k = 0u; k < 16u; ++k)
        if (at + k < n) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8u * (k & 3u)))) | ((uint32_t)text[at + k] << (8u * (k & 3u)));
}
__device__ __forceinline__ uint32_t bs_byte(const uint32_t w[4], const uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// a 256-lane workgroup's scan of the lanes' functions: returns the function of the lanes before this one, *total that of all of them
__device__ __forceinline__ uint32_t bs_block_prefix(const uint32_t f, uint32_t* lds4, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = f;
    for (uint32_t o = 1u; o < 64u; o <<= 1) { const uint32_t t = __shfl_up( inc, o, 64 ); if (lane >= o) inc = bs_compose( t, inc ); }
    if (lane == 63u) lds4[wave] = inc;
    __syncthreads();
    uint32_t ex = __shfl_up( inc, 1, 64 );
    if (lane == 0u) ex = BS_IDENTITY;
    uint32_t pre = BS_IDENTITY, tot = BS_IDENTITY;
    for (uint32_t w = 0u; w < 4u; ++w) { const uint32_t t = lds4[w]; if (w < wave) pre = bs_compose( pre, t ); tot = bs_compose( tot, t ); }
    *total = tot;
    __syncthreads();
    return bs_compose( pre, ex );
}

__device__ __forceinline__ uint32_t bs_shfl_up(const uint32_t v, const uint32_t o) { return __shfl_up( v, o, 64 ); }

// ONE 1024-lane workgroup's exclusive scan of vals[0, n) in place under the associative `op` with identity `id`; returns the total.
// T needs a bs_shfl_up overload; part: 16 T in LDS.
template <typename T, typename Op>
__device__ __forceinline__ T bs_scan_in_place(T* __restrict__ vals, const uint32_t n, const T id, const Op op, T* part)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint64_t b64 = (uint64_t)tid * chunk;
    const uint32_t b = b64 < n ? (uint32_t)b64 : n, e = n - b < chunk ? n : b + chunk;
    T acc = id;
    for (uint32_t i = b; i < e; ++i) acc = op( acc, vals[i] );
    T inc = acc;
    for (uint32_t o = 1u; o < 64u; o <<= 1) { const T t = bs_shfl_up( inc, o ); if (lane >= o) inc = op( t, inc ); }
    if (lane == 63u) part[wave] = inc;
    __syncthreads();
    T ex = bs_shfl_up( inc, 1u );
    if (lane == 0u) ex = id;
    T pre = id, tot = id;
    for (uint32_t w = 0u; w < 16u; ++w) { const T t = part[w]; if (w < wave) pre = op( pre, t ); tot = op( tot, t ); }
    T run = op( pre, ex );
    for (uint32_t i = b; i < e; ++i) { const T x = vals[i]; vals[i] = run; run = op( run, x ); }
    return tot;
}

} // namespace nvbio_amd
