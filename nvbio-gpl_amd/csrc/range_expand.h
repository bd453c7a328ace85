// range_expand.h -- the expansion of a list of ranges into one output per range element, shared by the FM, MEM and q-gram filters.
//
// A filter's rank leaves n ranges and `slots`, the inclusive uint64 scan of their sizes: output o of [0, slots[n-1]) belongs to range
// i = upper_bound( slots, o ) and is element o - slots[i-1] of it (o - 0 for i = 0).  The expansion gives a workgroup a tile of
// consecutive outputs; their ranges form a contiguous slice of `slots`, which two lanes bound with one binary search each, so that
// every output's own upper_bound runs over a few cached entries instead of log2( n ) HBM round trips, and a range of 10^4 elements
// is spread over 10^4 lanes.  What an output is -- a located text position, an index entry, a seed -- is the caller's functor.
#pragma once
#include "common.h"

namespace nvbio_amd {

// first i in [lo, hi) with a[i] > v (hi if none)
__device__ __forceinline__ uint32_t upper_bound_u64(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, const uint64_t v)
{
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// first i in [lo, hi) with a[i] >= v (hi if none)
__device__ __forceinline__ uint32_t lower_bound_u64(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, const uint64_t v)
{
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the size of a closed range [x, y] (an FM range: a uint2, or the first two words of a MEM's uint4); empty when y = x - 1
struct RangeSize
{
    template <typename R>
    __host__ __device__ __forceinline__ uint64_t operator()(const R r) const { return (uint64_t)(uint32_t)(1u + r.y - r.x); }
};

// the outputs of a tile: eight per lane of a 256-thread workgroup
constexpr uint32_t EXPAND_TILE = 256u * 8u;

// the grid of an expansion of the outputs [begin, end): a workgroup per tile (the kernels stride over the rest)
static inline unsigned expand_grid(const uint64_t begin, const uint64_t end)
{
    return grid_for( (end - begin + EXPAND_TILE - 1u) / EXPAND_TILE * 256u );
}

// the slice of `slots` that holds the ranges of a tile's outputs
struct TileSlots
{
    const uint64_t* slots;
    uint32_t        lo, hi;
    // the range of output o, and base = the outputs before that range
    __device__ __forceinline__ uint32_t find(const uint64_t o, uint64_t& base) const
    {
        const uint32_t i = upper_bound_u64( slots, lo, hi, o );
        base = i ? slots[i - 1u] : 0ull;
        return i;
    }
};

// body( t_first, t_end, TileSlots ) for every tile [t_first, t_end) of the outputs [begin, end) that falls to this workgroup (of 256
// threads, all of which must call); begin < end <= slots[n - 1]
template <uint32_t TILE = EXPAND_TILE, typename Body>
__device__ __forceinline__ void for_each_tile(const uint64_t* __restrict__ slots, const uint32_t n, const uint64_t begin, const uint64_t end, Body body)
{
    __shared__ uint32_t s_q[2];
    const uint64_t n_tiles = (end - begin + TILE - 1u) / TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        const uint64_t t_first = begin + tile * TILE;
        const uint64_t t_end   = (t_first + TILE < end) ? t_first + TILE : end;
        __syncthreads();
        if (threadIdx.x < 2) s_q[threadIdx.x] = upper_bound_u64( slots, 0u, n, threadIdx.x ? t_end - 1u : t_first );
        __syncthreads();
        body( t_first, t_end, TileSlots{ slots, s_q[0], s_q[1] + 1u < n ? s_q[1] + 1u : n } );
    }
}

// f( o, i, base ) for every output o of [begin, end): i its range, base the outputs before that range.  One lane per output.
template <uint32_t TILE = EXPAND_TILE, typename F>
__device__ __forceinline__ void expand_ranges(const uint64_t* __restrict__ slots, const uint32_t n, const uint64_t begin, const uint64_t end, F f)
{
    for_each_tile<TILE>( slots, n, begin, end, [&](const uint64_t t_first, const uint64_t t_end, const TileSlots ts)
    {
        for (uint64_t o = t_first + threadIdx.x; o < t_end; o += 256u)
        {
            uint64_t base;
            const uint32_t i = ts.find( o, base );
            f( o, i, base );
        }
    } );
}

} // namespace nvbio_amd
