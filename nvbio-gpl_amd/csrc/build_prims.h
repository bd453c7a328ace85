// build_prims.h -- the rocPRIM steps the suffix sorters share (fm_build.hip: one text; sufsort.hip: a string set): an in-place
// max-scan, the selection of the indices a predicate holds for, and a pair sort that brings its own temporary.  Each takes the
// build's buffers as `bufs`, synchronizes, and gives its temporaries back.
#pragma once
#include "common.h"
#include <rocprim/rocprim.hpp>

namespace nvbio_amd {

struct MaxU32
{
    __device__ __host__ __forceinline__ uint32_t operator()(const uint32_t a, const uint32_t b) const { return a > b ? a : b; }
};

static __global__ void patch_first_kernel(uint32_t* p, const uint32_t* carry) { if (*carry > *p) *p = *carry; }

// inclusive max-scan in place, in chunks small enough for 32-bit-sized device primitives
static nvbio_status scan_max_inplace(uint32_t* buf, uint64_t n, BuildBuffers& bufs, hipStream_t s)
{
    const uint64_t CHUNK = 1ull << 30;
    size_t temp_bytes = 0;
    NVB_HIP( rocprim::inclusive_scan( nullptr, temp_bytes, buf, buf, (size_t)(n < CHUNK ? n : CHUNK), MaxU32(), s ) );
    NVB_ALLOC( temp, uint8_t, temp_bytes );
    for (uint64_t b = 0; b < n; b += CHUNK)
    {
        const size_t len = (size_t)((n - b) < CHUNK ? (n - b) : CHUNK);
        if (b) NVB_CHECK( NVB_LAUNCH( patch_first_kernel, dim3(1), dim3(1), s, buf + b, buf + b - 1 ) );
        NVB_HIP( rocprim::inclusive_scan( temp, temp_bytes, buf + b, buf + b, len, MaxU32(), s ) );
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    bufs.release( temp );
    return NVBIO_OK;
}

// out[0..count) = { i in [0,n) : pred(i) } in increasing order, chunked; *count on the host
template <typename Pred>
static nvbio_status select_indices(const uint64_t n, Pred pred, uint32_t* out, uint64_t* count, BuildBuffers& bufs, hipStream_t s)
{
    const uint64_t CHUNK = 1ull << 30;
    NVB_ALLOC( d_cnt, size_t, 1 );
    size_t temp_bytes = 0;
    NVB_HIP( rocprim::select( nullptr, temp_bytes, rocprim::counting_iterator<uint32_t>( 0 ), out, d_cnt,
                              (size_t)(n < CHUNK ? n : CHUNK), pred, s ) );
    NVB_ALLOC( temp, uint8_t, temp_bytes );
    uint64_t total = 0;
    for (uint64_t b = 0; b < n; b += CHUNK)
    {
        const size_t len = (size_t)((n - b) < CHUNK ? (n - b) : CHUNK);
        NVB_HIP( rocprim::select( temp, temp_bytes, rocprim::counting_iterator<uint32_t>( (uint32_t)b ), out + total, d_cnt, len, pred, s ) );
        size_t c = 0;
        NVB_HIP( hipMemcpyAsync( &c, d_cnt, sizeof(size_t), hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        total += c;
    }
    *count = total;
    bufs.release( temp ); bufs.release( d_cnt );
    return NVBIO_OK;
}

// (keys_in, vals_in) stably sorted over the key bits [begin_bit, end_bit) into (keys_out, vals_out)
template <typename KeyIn, typename K, typename ValIn, typename V>
static nvbio_status sort_pairs(KeyIn keys_in, K* keys_out, ValIn vals_in, V* vals_out, size_t n,
                               unsigned begin_bit, unsigned end_bit, BuildBuffers& bufs, hipStream_t s)
{
    size_t temp_bytes = 0;
    NVB_HIP( rocprim::radix_sort_pairs( nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s ) );
    NVB_ALLOC( temp, uint8_t, temp_bytes );
    NVB_HIP( rocprim::radix_sort_pairs( temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    bufs.release( temp );
    return NVBIO_OK;
}

} // namespace nvbio_amd
