// qgroup_inl.h -- the q-group index (the PEANUT structure) for gfx950, included by qgram.hip: a string index and a set index behind the
// q-gram handle, so that nvbio_qgram_ranges and the q-gram filter run over either kind of index.
//
// Reference behaviour reproduced (file:line relative to the reference tree):
//   QGroupIndexViewCore::range                         nvbio/qgram/qgroup.h:112-130
//   QGroupIndexDevice::build                           nvbio/qgram/qgroup_inl.h:162-277 (setup_I 28-63, setup_SS 67-109, setup_P 113-158)
//   uniform_seeds_functor (the set form, as QGramSetIndexDevice takes it)  nvbio/strings/seeds.h:88-118
//
// The structure, with A = 1 << symbol_size and W = A^q / 32:
//   I[W + 1]   bit (g & 31) of word g / 32 is set iff q-gram g occurs
//   S[W + 1]   the exclusive scan of popc( I[i] )
//   SS[n_unique + 1]  the exclusive scan of the occurrence counts of the unique q-grams in ascending numeric order
//   P[n_qgrams]       the occurrences: uint32 positions (string), uint2 (string_id, string_pos) (set)
//   range(g)   (0, 0) if the bit is clear, else the half-open (SS[r], SS[r + 1]) with r = S[i] + popc( I[i] & ((1 << j) - 1) )
// Packing, padding and N -> A are those of the q-gram index (qgram.hip): qgram_at and the seed count / enumerate kernels are reused.
//
// Layout.  I[i] and S[i] are kept interleaved as one uint2 array, so a lookup is two dependent gathers whatever the text size: the
// 8-byte (bits, rank) pair from one line, then the two adjacent SS words.  nvbio_qgroup_index_export hands them out as two arrays.
//
// Departures from the reference:
//   slot order  the reference's fill takes its slots with a returning atomic, so the order of a q-gram's occurrences in P is
//               whatever the scheduler made it.  Here it is defined: ascending position (string), string-major then position (set).
//               So SS equals the q-gram index's slots, P its index, and the set bits of I its qgrams; two builds give equal bytes.
//   range       g >= A^q is a miss (the reference reads I out of bounds).
//   n_unique    S[W] + popc( I[W] ).  The reference takes S[W]: right when A^q is a multiple of 32, where word W holds no bit, and
//               0 for q * symbol_size < 5, where W = 0 and the one word holds every bit.
//   empty       an empty text or set builds: n_unique = 0, SS = {0}.
//
// The build counts, it does not sort n keys.  Separate launches, so that a kernel boundary orders one pass against the next:
//   0  extract the q-grams (qgram_extract_kernel / the seed kernels of qgram.hip) into keys[n]
//   1  zero the table (memset); qgroup_mark_kernel ORs the bits, non-returning, device scope
//   2  rocprim::exclusive_scan of popc( table[i].x ) into the .y halves (a transform input and an output iterator that writes .y)
//   3  zero SS (memset); qgroup_count_kernel adds the occurrence counts, non-returning
//   4  rocprim::exclusive_scan of SS in place; a copy of it becomes the fill's cursors
//   5  qgroup_fill_kernel takes slots with a returning atomicAdd on the cursor and writes P
//   6  qgroup_order_kernel makes each slot's order the defined one, by size class: slots of one entry are skipped; up to 16 entries
//      one lane sorts in place by insertion (a scan of the slot when it is ordered already); larger slots go on a list that
//      rocprim::segmented_radix_sort_keys sorts, and slots of 2^18 entries or more on a second list the host sorts one by one with
//      the device-wide radix sort (a segmented sort gives one workgroup to a segment).  Both sort from a copy of P back into P, so
//      the unlisted slots stay as they are; a text without large slots (a random genome) makes no copy and runs no sort.
//      A set index keeps P as uint64 keys (string_id << 32 | string_pos) until qgroup_unkey_kernel turns them into uint2.
//
// Contention.  A homopolymer or tandem repeat sends thousands of consecutive positions to one word, and one word takes about 88
// returning atomics per microsecond chip-wide.  Consecutive positions are neighbouring lanes, so in passes 1, 3 and 5 the lanes of a
// wave that hold equal q-grams in a row form a run (wave_run: one shuffle, one ballot): the run's first lane alone reads the
// table, issues ONE atomic with the run's length, and the lanes take their offsets from it.  An all-A text costs one atomic per
// wave instead of 64, and the entries of a run land in ascending order, so most slots come out ordered before pass 6.
//
// Extraction cost.  The q-gram of a position is needed in passes 1, 3 and 5.  They are extracted once and kept as n x 8 bytes in a
// build buffer, not recomputed: the three passes then stream 8 bytes per position, which is little against their random atomics,
// and one set of kernels serves the string and the set form, whose enumeration (the shared range expansion plus the string bounds)
// is the costlier one to repeat.  The buffer is freed before the handle is returned.
//
// Storage: BuildBuffers / NVB_ALLOC only; the table, SS and P are handed to the handle.  No ScratchBlock site.
// Registers (gfx950 code object, -Rpass-analysis=kernel-resource-usage): VGPRs range 8, mark 12, count 20, fill 24, order 14-16,
// unkey 6, split 10; private_segment_fixed_size = 0 (no scratch, no private arrays) for every one.
// Measured (scripts/bench_qgroup.py): at 100 Mbp, Q = 16, the counting build takes 24.7 ms against the sort's 6.7 ms and
// the lookup ranks as fast as the sorted index's, not faster; the structure is for texts where the sorted search grows.
#pragma once

namespace nvbio_amd {

struct QGroupView
{
    const uint2*    table;
    const uint32_t* ss;
    uint64_t        n_codes;     // A^q
};

// the rank of q-gram bit j of a (bits, rank) pair among the unique q-grams
__device__ __forceinline__ uint32_t qgroup_slot(const uint2 w, const uint32_t j) { return w.y + __popc( w.x & ((1u << j) - 1u) ); }

// range( g ) (qgroup.h:112-130): half-open slots of g, (0, 0) on a miss
__device__ __forceinline__ uint2 qgroup_range(const QGroupView& v, const uint64_t g)
{
    if (g >= v.n_codes) return make_uint2( 0u, 0u );
    const uint2    w = v.table[g >> 5];
    const uint32_t j = (uint32_t)g & 31u;
    if (!((w.x >> j) & 1u)) return make_uint2( 0u, 0u );
    const uint32_t r = qgroup_slot( w, j );
    return make_uint2( v.ss[r], v.ss[r + 1u] );
}

__global__ void __launch_bounds__(256)
qgroup_range_kernel(const QGroupView v, const uint64_t* __restrict__ queries, const uint32_t n, uint2* __restrict__ ranges)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        ranges[i] = qgroup_range( v, queries[i] );
}

// The run of equal q-grams a lane belongs to among the consecutive lanes of its wave: head = the lane is its first, lead = the
// first lane, len = its length (in the head).  Every lane of the wave calls it; the lanes past the end of the input are inactive
// (they are the last ones of the last wave) and each is a run of its own.
struct WaveRun { uint32_t lead, len; bool head; };
__device__ __forceinline__ WaveRun wave_run(const uint64_t g, const bool active)
{
    const uint32_t lane = __lane_id();
    const uint64_t prev = __shfl_up( (unsigned long long)g, 1u );
    WaveRun r;
    r.head = lane == 0u || !active || prev != g;
    const uint64_t heads = __ballot( r.head );
    r.lead = 63u - (uint32_t)__clzll( (long long)(heads & (~0ull >> (63u - lane))) );
    const uint64_t above = (heads >> lane) >> 1;
    r.len = above ? (uint32_t)__ffsll( (unsigned long long)above ) : 64u - lane;
    return r;
}

// The kernels of passes 1, 3 and 5 walk the input in steps of the grid from a block-uniform base, so that every lane of a wave makes
// the same number of steps (wave_run needs them all): entry i = base + threadIdx.x, active while i < n.
// pass 1: set the bit of every q-gram
__global__ void __launch_bounds__(256)
qgroup_mark_kernel(const uint64_t* __restrict__ keys, const uint32_t n, uint2* __restrict__ table)
{
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const bool active = i < n;
        const uint64_t g = active ? keys[i] : 0u;
        const WaveRun run = wave_run( g, active );
        if (active && run.head) atomicOr( &table[g >> 5].x, 1u << ((uint32_t)g & 31u) );
    }
}

// pass 3: ss[r] += the occurrences of the r-th unique q-gram
__global__ void __launch_bounds__(256)
qgroup_count_kernel(const uint64_t* __restrict__ keys, const uint32_t n, const uint2* __restrict__ table, uint32_t* __restrict__ ss)
{
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const bool active = i < n;
        const uint64_t g = active ? keys[i] : 0u;
        const WaveRun run = wave_run( g, active );
        if (active && run.head) atomicAdd( &ss[qgroup_slot( table[g >> 5], (uint32_t)g & 31u )], run.len );
    }
}

// pass 5: P[slot] = the coordinate of entry i, its position (K = uint32) or the key string_id << 32 | string_pos of coords[i]
// (K = uint64); a run takes its slots with one atomic on the q-gram's cursor
template <typename K>
__global__ void __launch_bounds__(256)
qgroup_fill_kernel(const uint64_t* __restrict__ keys, const uint2* __restrict__ coords, const uint32_t n, const uint2* __restrict__ table,
                   uint32_t* __restrict__ cursor, K* __restrict__ P)
{
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const bool active = i < n;
        const uint64_t g = active ? keys[i] : 0u;
        const WaveRun run = wave_run( g, active );
        uint32_t at = 0u;
        if (active && run.head) at = atomicAdd( &cursor[qgroup_slot( table[g >> 5], (uint32_t)g & 31u )], run.len );
        at = __shfl( at, (int)run.lead ) + (__lane_id() - run.lead);
        if (active)
        {
            if (sizeof(K) == 4) P[at] = (K)i;
            else { const uint2 c = coords[i]; P[at] = (K)(((uint64_t)c.x << 32) | c.y); }
        }
    }
}

// pass 6: the entries of every slot in ascending order.  One entry: nothing to do.  Up to SMALL: this lane, by insertion in place.
// Larger: the slot's [begin, end) goes on the list of segments (n_lists[0] of them) or, from HUGE entries on, on the list of huge
// slots (n_lists[1]) for the host to sort.
static const uint32_t QGROUP_SMALL = 16u, QGROUP_HUGE = 1u << 18;
template <typename K>
__global__ void __launch_bounds__(256)
qgroup_order_kernel(const uint32_t* __restrict__ ss, const uint32_t n_unique, K* __restrict__ P, uint32_t* __restrict__ seg_begin,
                    uint32_t* __restrict__ seg_end, uint2* __restrict__ huge, uint32_t* __restrict__ n_lists)
{
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n_unique; u += gridDim.x * blockDim.x)
    {
        const uint32_t b = ss[u], e = ss[u + 1u], len = e - b;
        if (len < 2u) continue;
        if (len <= QGROUP_SMALL)
        {
            for (uint32_t a = b + 1u; a < e; ++a)
            {
                const K x = P[a];
                uint32_t c = a;
                while (c > b && P[c - 1u] > x) { P[c] = P[c - 1u]; --c; }
                if (c != a) P[c] = x;
            }
        }
        else if (len < QGROUP_HUGE)
        {
            const uint32_t k = atomicAdd( &n_lists[0], 1u );
            seg_begin[k] = b; seg_end[k] = e;
        }
        else huge[atomicAdd( &n_lists[1], 1u )] = make_uint2( b, e );
    }
}

// a set index's keys string_id << 32 | string_pos into its coordinates (string_id, string_pos), in place
__global__ void __launch_bounds__(256)
qgroup_unkey_kernel(uint64_t* __restrict__ P, const uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const uint64_t k = P[i];
        ((uint2*)P)[i] = make_uint2( (uint32_t)(k >> 32), (uint32_t)k );
    }
}

// the interleaved table as the reference's two arrays (either may be NULL)
__global__ void __launch_bounds__(256)
qgroup_split_kernel(const uint2* __restrict__ table, const uint64_t n_words, uint32_t* __restrict__ I, uint32_t* __restrict__ S)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint2 w = table[i];
        if (I) I[i] = w.x;
        if (S) S[i] = w.y;
    }
}

struct QGroupPopcount
{
    __host__ __device__ __forceinline__ uint32_t operator()(const uint2 w) const { return (uint32_t)__builtin_popcount( w.x ); }
};

// a write-only iterator over the rank halves of the table: *it = v stores table[i].y = v and leaves the bits alone
class QGroupRankIterator
{
public:
    struct proxy_type
    {
        uint2* p;
        __host__ __device__ __forceinline__ proxy_type operator=(const uint32_t v) { p->y = v; return *this; }
    };
    using value_type = void;
    using reference = void;
    using pointer = void;
    using difference_type = std::ptrdiff_t;
    using iterator_category = std::output_iterator_tag;
    __host__ __device__ explicit QGroupRankIterator(uint2* p) : p_( p ) {}
    __host__ __device__ QGroupRankIterator& operator++() { ++p_; return *this; }
    __host__ __device__ QGroupRankIterator operator++(int) { QGroupRankIterator o = *this; ++p_; return o; }
    __host__ __device__ proxy_type operator*() const { return proxy_type{ p_ }; }
    __host__ __device__ proxy_type operator[](const difference_type d) const { return proxy_type{ p_ + d }; }
    __host__ __device__ QGroupRankIterator operator+(const difference_type d) const { return QGroupRankIterator( p_ + d ); }
    __host__ __device__ QGroupRankIterator& operator+=(const difference_type d) { p_ += d; return *this; }
    __host__ __device__ QGroupRankIterator operator-(const difference_type d) const { return QGroupRankIterator( p_ - d ); }
    __host__ __device__ QGroupRankIterator& operator-=(const difference_type d) { p_ -= d; return *this; }
private:
    uint2* p_;
};

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static nvbio_status check_qgroup_params(const uint32_t q, const uint32_t ss)
{
    NVB_REQUIRE( ss >= 1 && ss <= 8, "symbol_size must be in [1, 8]" );
    NVB_REQUIRE( q >= 1 && (uint64_t)q * ss <= 36, "q must be >= 1 with q * symbol_size <= 36 (the q-group table holds A^q bits)" );
    return NVBIO_OK;
}

static QGroupView group_view_of(const nvbio_qgram_index_s* h)
{
    QGroupView v;
    v.table = h->table; v.ss = h->slots; v.n_codes = 1ull << (h->q * h->symbol_size);
    return v;
}

// ranges[i] = range( queries[i] ) through the lookup of the handle's kind
static nvbio_status launch_ranges(const nvbio_qgram_index_s* h, const uint64_t* queries, const uint32_t n, uint2* ranges, hipStream_t s)
{
    if (h->is_group) return NVB_LAUNCH( qgroup_range_kernel, dim3( grid_for( n ) ), dim3(256), s, group_view_of( h ), queries, n, ranges );
    return NVB_LAUNCH( qgram_range_kernel, dim3( grid_for( n ) ), dim3(256), s, view_of( h ), queries, n, ranges );
}

// the exclusive scan of n uint32 values from `in` to `out` with a temp of `bufs`
template <typename In, typename Out>
static nvbio_status qgroup_scan(BuildBuffers& bufs, In in, Out out, const uint64_t n, hipStream_t s)
{
    size_t a = 0;
    NVB_HIP( rocprim::exclusive_scan( nullptr, a, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s ) );
    NVB_ALLOC( temp, uint8_t, a );
    NVB_HIP( rocprim::exclusive_scan( temp, a, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    bufs.release( temp );
    return NVBIO_OK;
}

// the position of the highest set bit of x, plus one (0 for 0)
static uint32_t bit_length(const uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll( x ) : 0u; }

// pass 6 behind qgroup_order_kernel: sort the listed slots of P (n keys of key_bits significant bits) from a copy of P
template <typename K>
static nvbio_status sort_listed_slots(BuildBuffers& bufs, K* P, const uint32_t n, const uint32_t key_bits, const uint32_t* seg_begin,
                                      const uint32_t* seg_end, const uint32_t n_segs, const uint2* huge_dev, const uint32_t n_huge, hipStream_t s)
{
    if (n_segs == 0 && n_huge == 0) return NVBIO_OK;
    NVB_ALLOC( copy, K, n );
    NVB_HIP( hipMemcpyAsync( copy, P, sizeof(K) * (uint64_t)n, hipMemcpyDeviceToDevice, s ) );
    if (n_segs)
    {
        size_t a = 0;
        NVB_HIP( rocprim::segmented_radix_sort_keys( nullptr, a, (const K*)copy, P, (size_t)n, n_segs, seg_begin, seg_end, 0u, key_bits, s ) );
        NVB_ALLOC( temp, uint8_t, a );
        NVB_HIP( rocprim::segmented_radix_sort_keys( temp, a, (const K*)copy, P, (size_t)n, n_segs, seg_begin, seg_end, 0u, key_bits, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp );
    }
    if (n_huge)
    {
        std::vector<uint2> huge( n_huge );
        NVB_HIP( hipMemcpyAsync( huge.data(), huge_dev, 8ull * n_huge, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        size_t a = 0;
        NVB_HIP( rocprim::radix_sort_keys( nullptr, a, (const K*)copy, P, (size_t)n, 0u, key_bits, s ) );
        NVB_ALLOC( temp, uint8_t, a );
        for (const uint2 h : huge)
        {
            size_t bytes = a;
            NVB_HIP( rocprim::radix_sort_keys( temp, bytes, (const K*)copy + h.x, P + h.x, (size_t)(h.y - h.x), 0u, key_bits, s ) );
        }
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp );
    }
    bufs.release( copy );
    return NVBIO_OK;
}

// passes 1-6 over the n extracted q-grams in keys (and, for a set index, their coordinates in coords); hands the table, SS and P
// to a new handle.  K is uint32 (string: the coordinate of entry i is i) or uint64 (set).  max_coord: the largest key P can hold.
template <typename K>
static nvbio_status build_qgroup(BuildBuffers& bufs, const int device, const uint32_t q, const uint32_t ss, const uint32_t n, uint64_t* keys,
                                 uint64_t* coords, const uint64_t max_coord, hipStream_t s, nvbio_qgram_index_t* out)
{
    const uint64_t n_words = (1ull << (q * ss)) / 32u + 1u;
    const dim3 grid( grid_for( n ) ), block( 256 );
    // 1: the bits
    NVB_ALLOC( table, uint2, n_words );
    NVB_HIP( hipMemsetAsync( table, 0, 8ull * n_words, s ) );
    if (n) NVB_CHECK( NVB_LAUNCH( qgroup_mark_kernel, grid, block, s, (const uint64_t*)keys, n, table ) );
    // 2: the ranks
    NVB_CHECK( qgroup_scan( bufs, rocprim::transform_iterator<const uint2*, QGroupPopcount, uint32_t>( table, QGroupPopcount() ),
                            QGroupRankIterator( table ), n_words, s ) );
    uint2 last;
    NVB_HIP( hipMemcpyAsync( &last, table + (n_words - 1u), 8, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    const uint32_t n_unique = last.y + (uint32_t)__builtin_popcount( last.x );
    // 3, 4: the slots
    NVB_ALLOC( slots, uint32_t, n_unique + 1ull );
    NVB_HIP( hipMemsetAsync( slots, 0, 4ull * (n_unique + 1ull), s ) );
    if (n) NVB_CHECK( NVB_LAUNCH( qgroup_count_kernel, grid, block, s, (const uint64_t*)keys, n, (const uint2*)table, slots ) );
    NVB_CHECK( qgroup_scan( bufs, slots, slots, n_unique + 1ull, s ) );
    // 5: the occurrences
    NVB_ALLOC( P, K, n );
    if (n)
    {
        NVB_ALLOC( cursor, uint32_t, n_unique );
        NVB_HIP( hipMemcpyAsync( cursor, slots, 4ull * n_unique, hipMemcpyDeviceToDevice, s ) );
        NVB_CHECK( NVB_LAUNCH( qgroup_fill_kernel<K>, grid, block, s, (const uint64_t*)keys, (const uint2*)coords, n, (const uint2*)table, cursor, P ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( cursor );
    }
    bufs.release( keys );
    if (coords) bufs.release( coords );
    // 6: the order inside the slots
    if (n)
    {
        NVB_ALLOC( seg_begin, uint32_t, n / (QGROUP_SMALL + 1u) + 1u );
        NVB_ALLOC( seg_end, uint32_t, n / (QGROUP_SMALL + 1u) + 1u );
        NVB_ALLOC( huge, uint2, n / QGROUP_HUGE + 1u );
        NVB_ALLOC( n_lists, uint32_t, 2 );
        NVB_HIP( hipMemsetAsync( n_lists, 0, 8, s ) );
        NVB_CHECK( NVB_LAUNCH( qgroup_order_kernel<K>, dim3( grid_for( n_unique ) ), block, s, (const uint32_t*)slots, n_unique, P, seg_begin, seg_end,
                               huge, n_lists ) );
        uint32_t counts[2] = { 0u, 0u };
        NVB_HIP( hipMemcpyAsync( counts, n_lists, 8, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        NVB_CHECK( sort_listed_slots<K>( bufs, P, n, bit_length( max_coord ), seg_begin, seg_end, counts[0], huge, counts[1], s ) );
        bufs.release( seg_begin ); bufs.release( seg_end ); bufs.release( huge ); bufs.release( n_lists );
        if (sizeof(K) == 8) NVB_CHECK( NVB_LAUNCH( qgroup_unkey_kernel, grid, block, s, (uint64_t*)P, n ) );
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    nvbio_qgram_index_s* h = new (std::nothrow) nvbio_qgram_index_s();
    if (!h) { set_error( "out of host memory" ); return NVBIO_ERR_NOMEM; }
    h->device = device; h->q = q; h->symbol_size = ss; h->is_set = sizeof(K) == 8 ? 1u : 0u;
    h->n_qgrams = n; h->n_unique = n_unique;
    h->slots = slots; h->index = P; h->is_group = 1u; h->table = table; h->n_words = n_words;
    h->bytes = 8ull * n_words + 4ull * (n_unique + 1ull) + sizeof(K) * (uint64_t)n;
    bufs.forget( table ); bufs.forget( slots ); bufs.forget( P );
    *out = h;
    return NVBIO_OK;
}

} // namespace nvbio_amd

extern "C" {

nvbio_status nvbio_qgroup_index_build(int device, const void* text_dev, uint32_t text_bits, uint32_t length, uint32_t q, uint32_t symbol_size,
                                      nvbio_qgram_index_t* out, void* stream)
{
    using namespace nvbio_amd;
    NVB_REQUIRE( out != nullptr, "out is NULL" );
    *out = nullptr;
    NVB_CHECK( check_text_bits( text_bits ) );
    NVB_CHECK( check_qgroup_params( q, symbol_size ) );
    NVB_REQUIRE( length == 0 || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( length < 0xFFFFFFFFu, "length must be below 2^32 - 1" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    BuildBuffers bufs( "q-group index build" );
    NVB_ALLOC( keys, uint64_t, length );
    if (length)
    {
        NVB_CHECK( with_value( SymbolBits(), text_bits, [&](auto BITS)
        {
            return NVB_LAUNCH( qgram_extract_kernel<BITS>, dim3( grid_for( length ) ), dim3(256), s, text_dev, length, q, symbol_size, 0u,
                               length, keys, (uint32_t*)nullptr );
        }, bad_symbol_bits ) );
    }
    return build_qgroup<uint32_t>( bufs, device, q, symbol_size, length, keys, nullptr, length ? length - 1u : 0u, s, out );
}

nvbio_status nvbio_qgroup_set_index_build(int device, const nvbio_string_set* set, uint32_t q, uint32_t symbol_size, uint32_t seed_interval,
                                          nvbio_qgram_index_t* out, void* stream)
{
    using namespace nvbio_amd;
    NVB_REQUIRE( out != nullptr && set != nullptr, "NULL argument" );
    *out = nullptr;
    NVB_CHECK( check_text_bits( set->symbol_bits ) );
    NVB_CHECK( check_qgroup_params( q, symbol_size ) );
    NVB_CHECK( check_plain_set( set, seed_interval ) );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    BuildBuffers bufs( "q-group index build" );
    uint32_t n = 0; uint64_t* keys = nullptr; uint64_t* coords = nullptr;
    NVB_CHECK( enumerate_set_seeds( bufs, set, q, symbol_size, seed_interval, s, n, keys, coords ) );
    return build_qgroup<uint64_t>( bufs, device, q, symbol_size, n, keys, coords, ((uint64_t)set->n << 32) | 0xFFFFFFFFull, s, out );
}

nvbio_status nvbio_qgroup_index_get_view(nvbio_qgram_index_t index, nvbio_qgroup_index_view* view)
{
    using namespace nvbio_amd;
    NVB_REQUIRE( index && view, "NULL argument" );
    NVB_REQUIRE( index->is_group, "not a q-group index" );
    view->q = index->q; view->symbol_size = index->symbol_size; view->is_set = index->is_set;
    view->n_qgrams = index->n_qgrams; view->n_unique = index->n_unique; view->n_words = index->n_words; view->device = index->device;
    view->table_dev = (const nvbio_uint2*)index->table; view->ss_dev = index->slots; view->p_dev = index->index;
    return NVBIO_OK;
}

nvbio_status nvbio_qgroup_index_export(nvbio_qgram_index_t index, uint32_t* I_out_dev, uint32_t* S_out_dev, uint32_t* SS_out_dev, void* P_out_dev,
                                       void* stream)
{
    using namespace nvbio_amd;
    NVB_REQUIRE( index != nullptr, "index is NULL" );
    NVB_REQUIRE( index->is_group, "not a q-group index" );
    DeviceGuard g( index->device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t w = index->is_set ? 8u : 4u;
    if (I_out_dev || S_out_dev)
        NVB_CHECK( NVB_LAUNCH( qgroup_split_kernel, dim3( grid_for( index->n_words ) ), dim3(256), s, (const uint2*)index->table, index->n_words,
                               I_out_dev, S_out_dev ) );
    if (SS_out_dev) NVB_HIP( hipMemcpyAsync( SS_out_dev, index->slots, 4ull * (index->n_unique + 1ull), hipMemcpyDeviceToDevice, s ) );
    if (P_out_dev && index->n_qgrams) NVB_HIP( hipMemcpyAsync( P_out_dev, index->index, w * index->n_qgrams, hipMemcpyDeviceToDevice, s ) );
    return NVBIO_OK;
}

} // extern "C"
