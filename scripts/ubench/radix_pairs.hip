// radix_pairs -- the cost of the reference's set suffix sorter on this chip, with rocPRIM alone: it sorts all n suffixes once per
// 14-symbol word, least significant word first, as (32-bit key, 32-bit value) pairs (nvbio/sufsort/sufsort_inl.h:70-135), i.e.
// `sorts` stable radix sorts of n pairs.  Key extraction is left out, so this is a lower bound of its time.
//   radix_pairs <n> <sorts> [steps]   ->  one JSON line; device events around the `sorts` sorts, after one warm-up, median of steps
#include <cstdint>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf( stderr, "%s: %s\n", #x, hipGetErrorString( e ) ); return 1; } } while (0)

__global__ void fill_kernel(uint32_t* keys, uint32_t* vals, const size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    {
        uint32_t x = (uint32_t)i * 2654435761u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        keys[i] = x & 0x0FFFFFFFu;                        // 14 two-bit symbols
        vals[i] = (uint32_t)i;
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf( stderr, "usage: %s n sorts [steps]\n", argv[0] ); return 2; }
    const size_t n = strtoull( argv[1], 0, 0 );
    const int sorts = atoi( argv[2] ), steps = argc > 3 ? atoi( argv[3] ) : 3;
    uint32_t *k0, *k1, *v0, *v1;
    CHECK( hipMalloc( &k0, n * 4 ) ); CHECK( hipMalloc( &k1, n * 4 ) ); CHECK( hipMalloc( &v0, n * 4 ) ); CHECK( hipMalloc( &v1, n * 4 ) );
    size_t temp_bytes = 0;
    CHECK( rocprim::radix_sort_pairs( nullptr, temp_bytes, k0, k1, v0, v1, n, 0u, 28u ) );
    void* temp; CHECK( hipMalloc( &temp, temp_bytes ) );
    hipEvent_t e0, e1; CHECK( hipEventCreate( &e0 ) ); CHECK( hipEventCreate( &e1 ) );
    std::vector<float> ms;
    for (int step = 0; step < steps + 1; ++step)
    {
        fill_kernel<<<4096, 256>>>( k0, v0, n );
        CHECK( hipGetLastError() );
        CHECK( hipEventRecord( e0 ) );
        for (int s = 0; s < sorts; ++s)
        {
            if (s & 1) CHECK( rocprim::radix_sort_pairs( temp, temp_bytes, k1, k0, v1, v0, n, 0u, 28u ) );
            else       CHECK( rocprim::radix_sort_pairs( temp, temp_bytes, k0, k1, v0, v1, n, 0u, 28u ) );
        }
        CHECK( hipEventRecord( e1 ) );
        CHECK( hipEventSynchronize( e1 ) );
        float t = 0; CHECK( hipEventElapsedTime( &t, e0, e1 ) );
        if (step) ms.push_back( t );
    }
    std::sort( ms.begin(), ms.end() );
    printf( "{\"n\": %zu, \"sorts\": %d, \"ms\": %.4f, \"temp_bytes\": %zu, \"bytes\": %zu}\n", n, sorts, ms[ms.size() / 2], temp_bytes, temp_bytes + 16 * n );
    return 0;
}
