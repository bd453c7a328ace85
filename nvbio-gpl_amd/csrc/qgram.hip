// qgram.hip -- q-gram seeding for gfx950: the q-gram string index, the q-gram string-set index and the q-gram filter (rank / locate /
// merge) behind the C ABI.  The q-group index, the O(1)-lookup alternative behind the same handle, is qgroup_inl.h, included below.
//
// Reference behaviour reproduced (file:line relative to the reference tree):
//   string_qgram_functor / string_set_qgram_functor   nvbio/qgram/qgram.h:793-886
//   QGramIndexDevice::build                           nvbio/qgram/qgram_inl.h:30-140
//   QGramSetIndexDevice::build + uniform_seeds_functor qgram_inl.h:186-300, nvbio/strings/seeds.h:88-118
//   QGramIndexViewCore::range                         qgram.h:451-475
//   QGramFilter<device_tag>::rank / locate / merge    nvbio/qgram/filter_inl.h:37-190, 336-483
//   build_qgrams (generate_qgrams + sort_by_key)      examples/qmap/qmap.cu:75-99
//
// The parity traps, restated:
//   packing  g = sum_j (s[i+j] & mask) << (j * symbol_size), mask = (1 << symbol_size) - 1: the FIRST symbol sits in the LEAST
//            significant bits (numeric order is not lexicographic order); positions past the end of the string contribute 0; a 4-bit
//            N (4) read with symbol_size 2 becomes A (qmap's "implicitly convert N to A").
//   string   every one of the string_len positions is indexed, the last Q-1 padded with 0 symbols: n_qgrams = string_len.  Stable radix
//            sort over bits [0, Q * symbol_size) of (q-gram, uint32 position) pairs in position order: the occurrences of one q-gram are
//            in ascending position order.  qgrams = the sorted unique q-grams, slots[n_unique + 1] = exclusive scan of their counts,
//            index[n_qgrams] = the occurrences.
//   set      seeds at pos = k * interval for every k with pos + q <= len (no padding), string-major then by position; coordinates
//            (string_id, string_pos) uint32 pairs, sorted stably in that order.
//   LUT      QLS = (Q - QL) * symbol_size; lut[k] = lower_bound( qgrams, k << QLS ) for k < A^QL, lut[A^QL] = n_unique: it keys on a
//            q-gram's TOP bits, i.e. its LAST QL symbols.
//   range    lower_bound inside the LUT bucket (over everything without a LUT); the HALF-OPEN [slots[i], slots[i+1]), a miss (0, 0).
//            (The FM ranges of this library are inclusive.)  A query with bits above Q * symbol_size equals no indexed q-gram and is
//            a miss here; the reference would index its LUT past the end.
//   rank     ranges[i] = range( queries[i] ); slots = INCLUSIVE uint64 scan of the range sizes; the hit count is slots[n - 1].
//   locate   output o belongs to query i = upper_bound( o, slots ); string index: (index[ranges[i].x + o - slots[i-1]], indices[i]), a
//            uint2 of (index position, query coordinate); set index: (string_id, string_pos, indices[i], 0), a uint4.
//   merge    diagonal = text_pos - index_pos (string) or text_pos - string_pos (set), in uint32 (it wraps), snapped to the interval
//            (see "Departures"); sorted as a primitive -- uint32 for string hits, uint64 = the uint2 (diagonal, string_id) for set
//            hits, so set output is ordered by string id, then diagonal -- and run-length encoded into (diagonal, count).
//
// Departures from the reference (reference defects, not reproduced):
//   rounding   util::round (nvbio/basic/numbers.h:149-153) returns r + 1 where its name and comment say "the closest multiple of
//              interval".  Here r = interval * floor(d / interval); snapped = (d - r) > interval - (d - r) ? r + interval : r, i.e.
//              2 (d - r) > interval without the doubling overflowing; in uint32 (mod 2^32).  With a power-of-two interval a diagonal
//              of -3 snaps to 0.  It matters downstream: qmap turns the snapped diagonal into a band-31 window, and with r + 1 a read
//              can land outside it.
//   no queries rank with n_queries = 0 returns 0 hits (the reference reads slots[-1]).
//   hit index  the set-index locate keeps base_slot / local_index 64-bit (the reference truncates them to 32 bits: wrong above 2^32 hits).
//   counts     merged counts are uint32 (qmap uses uint16, which a repeat can overflow).
//
// MI355X shape.  Range lookup is a chain of dependent random 8-byte loads: two LUT words, then a lower_bound inside the bucket, then
// the slots.  At qmap's shape (a set index of ~28 M seeds of 2 M reads, LUT 12 over 16.8 M buckets) a bucket holds about one entry
// and at a 100 Mbp string index about six, so the search is one to three steps and a wave-cooperative 64-ary search would spend 64
// lanes on what one lane finishes in as many dependent loads; one lane per query it is.  qmap feeds its queries sorted, so
// neighbouring lanes hit neighbouring buckets.  (At 3 Gbp, ~180 entries per bucket, the lane does ~8 steps; not measured.)
// Locate: one lane per output, as the reference, through the expansion the three filters share (range_expand.h): a workgroup first
// bounds the queries its 2,048 consecutive outputs belong to, so each output's own upper_bound runs over a few cached entries.
// Extraction, seed enumeration, LUT build and the diagonal snap are one lane per item.  No private arrays; sorting, scans and
// run-length encoding are rocPRIM.  Working storage: the index builds take BuildBuffers (their arrays are handed to the handle),
// generate_qgrams (sorted), rank and merge a ScratchBlock on the caller's temp.
// Registers (gfx950 code object, -Rpass-analysis=kernel-resource-usage): VGPRs extract 14-16, seed count 8, seed enumerate 26-28,
// LUT 11, range 11, locate 20, diagonal 9-10; private_segment_fixed_size = 0 (no scratch) for every one.
#include "range_expand.h"
#include <rocprim/rocprim.hpp>

struct nvbio_qgram_index_s
{
    int       device;
    uint32_t  q, symbol_size, qlut, is_set;
    uint32_t  n_qgrams, n_unique;
    uint64_t* qgrams;      // n_unique
    uint32_t* slots;       // n_unique + 1
    void*     index;       // n_qgrams uint32 positions, or uint2 (string_id, string_pos)
    uint32_t* lut;         // lut_size + 1, or NULL
    uint64_t  lut_size;    // A^QL (0 without a LUT)
    uint64_t  bytes;
    // a q-group index (qgroup_inl.h): slots = SS, index = P, qgrams = lut = NULL, qlut = 0
    uint32_t  is_group;
    uint2*    table;       // n_words interleaved (I[i], S[i]) pairs
    uint64_t  n_words;     // A^q / 32 + 1
};

namespace nvbio_amd {

struct QGramView
{
    const uint64_t* qgrams;
    const uint32_t* slots;
    const uint32_t* lut;
    uint64_t        lut_size;
    uint32_t        n_unique;
    uint32_t        qls;
};

// string i of a plain set: its first symbol and its length
struct QGramSet
{
    const void*     symbols;
    const uint32_t* offsets;
    uint32_t        ranges, fixed_len, stride, n;
    __device__ __forceinline__ void bounds(const uint32_t i, uint32_t& begin, uint32_t& len) const
    {
        if (offsets && ranges) { begin = offsets[i]; len = offsets[i + 1] - begin; }
        else                   { begin = offsets ? offsets[i] : i * stride; len = fixed_len; }
    }
};

// the q-gram of q symbols at [pos, pos + q) of a string at `begin` of length `len`, 0 past its end (string_qgram_functor)
template <int BITS>
__device__ __forceinline__ uint64_t qgram_at(SymbolReader<BITS>& rd, const uint64_t begin, const uint32_t len, const uint32_t pos,
                                             const uint32_t q, const uint32_t ss)
{
    const uint32_t mask = (1u << ss) - 1u;
    uint64_t g = 0;
    for (uint32_t j = 0; j < q; ++j)
    {
        const uint64_t p = (uint64_t)pos + j;
        if (p >= len) break;
        g |= (uint64_t)(rd.get( (uint32_t)(begin + p) ) & mask) << (j * ss);
    }
    return g;
}

// qgrams[i] = the q-gram at text position first + i (padded past len), pos[i] = first + i (pos may be NULL)
template <int BITS>
__global__ void __launch_bounds__(256)
qgram_extract_kernel(const void* text, const uint32_t len, const uint32_t q, const uint32_t ss, const uint32_t first, const uint32_t n,
                     uint64_t* __restrict__ qgrams, uint32_t* __restrict__ pos)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        SymbolReader<BITS> rd( text );
        const uint32_t p = first + i;
        qgrams[i] = qgram_at<BITS>( rd, 0u, len, p, q, ss );
        if (pos) pos[i] = p;
    }
}

// seeds of string i (uniform_seeds_functor( q, interval )): pos = k * interval, pos + q <= len
__global__ void __launch_bounds__(256)
qgram_seed_count_kernel(const QGramSet s, const uint32_t q, const uint32_t interval, uint64_t* __restrict__ cnt)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += gridDim.x * blockDim.x)
    {
        uint32_t begin, len;
        s.bounds( i, begin, len );
        cnt[i] = len >= q ? (uint64_t)(len - q) / interval + 1u : 0u;
    }
}

// seed k of the set (first[i] = exclusive scan of the seed counts, n + 1 entries): its coordinate and q-gram.  The shared expansion
// (range_expand.h) over tiles of 256 seeds: read as an inclusive scan, `first` has the empty range 0 in front of the strings' seeds,
// so seed k falls into range sid + 1 and `base` is first[sid].
template <int BITS>
__global__ void __launch_bounds__(256)
qgram_seed_enumerate_kernel(const QGramSet s, const uint32_t q, const uint32_t ss, const uint32_t interval, const uint64_t* __restrict__ first,
                            const uint32_t n_seeds, uint64_t* __restrict__ qgrams, uint2* __restrict__ coords)
{
    expand_ranges<256u>( first, s.n + 1u, 0u, n_seeds, [&](const uint64_t k, const uint32_t i, const uint64_t base)
    {
        const uint32_t sid = i - 1u;
        const uint32_t pos = (uint32_t)(k - base) * interval;
        uint32_t begin, len;
        s.bounds( sid, begin, len );
        SymbolReader<BITS> rd( s.symbols );
        qgrams[k] = qgram_at<BITS>( rd, begin, len, pos, q, ss );
        coords[k] = make_uint2( sid, pos );
    } );
}

// lut[k] = lower_bound( qgrams, k << qls ) for k < lut_size, lut[lut_size] = n_unique
__global__ void __launch_bounds__(256)
qgram_lut_kernel(const uint64_t* __restrict__ qgrams, const uint32_t n_unique, const uint32_t qls, const uint64_t lut_size, uint32_t* __restrict__ lut)
{
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k <= lut_size; k += (uint64_t)gridDim.x * blockDim.x)
        lut[k] = k < lut_size ? lower_bound_u64( qgrams, 0u, n_unique, k << qls ) : n_unique;
}

// range( g ) (qgram.h:451-475): half-open slots of g, (0, 0) on a miss
__device__ __forceinline__ uint2 qgram_range(const QGramView& v, const uint64_t g)
{
    uint32_t lo = 0u, hi = v.n_unique;
    if (v.lut)
    {
        const uint64_t k = g >> v.qls;
        if (k >= v.lut_size) return make_uint2( 0u, 0u );
        lo = v.lut[k]; hi = v.lut[k + 1u];
    }
    const uint32_t i = lower_bound_u64( v.qgrams, lo, hi, g );
    if (i >= v.n_unique || v.qgrams[i] != g) return make_uint2( 0u, 0u );
    return make_uint2( v.slots[i], v.slots[i + 1u] );
}

__global__ void __launch_bounds__(256)
qgram_range_kernel(const QGramView v, const uint64_t* __restrict__ queries, const uint32_t n, uint2* __restrict__ ranges)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        ranges[i] = qgram_range( v, queries[i] );
}

struct QGramRangeSize
{
    __host__ __device__ __forceinline__ uint64_t operator()(const uint2 r) const { return (uint64_t)(r.y - r.x); }
};

// locate (filter_results, filter_inl.h:88-190): hits[o - begin] for the outputs o in [begin, end), over the shared expansion
// (expand_ranges, range_expand.h)
template <bool SET>
__global__ void __launch_bounds__(256)
qgram_locate_kernel(const void* __restrict__ index, const uint2* __restrict__ ranges, const uint64_t* __restrict__ slots,
                    const uint32_t* __restrict__ indices, const uint32_t n, const uint64_t begin, const uint64_t end, void* __restrict__ hits)
{
    expand_ranges( slots, n, begin, end, [&](const uint64_t o, const uint32_t i, const uint64_t base)
    {
        const uint64_t at = (uint64_t)ranges[i].x + (o - base);
        if (SET)
        {
            const uint2 c = ((const uint2*)index)[at];
            ((uint4*)hits)[o - begin] = make_uint4( c.x, c.y, indices[i], 0u );
        }
        else ((uint2*)hits)[o - begin] = make_uint2( ((const uint32_t*)index)[at], indices[i] );
    } );
}

// the closest multiple of `interval` to d, ties down, mod 2^32 (see "Departures": rounding)
__device__ __forceinline__ uint32_t snap_diagonal(const uint32_t d, const uint32_t interval)
{
    const uint32_t r = (d / interval) * interval;
    const uint32_t x = d - r;
    return x > interval - x ? r + interval : r;
}

// closest_diagonal: string hits (index_pos, text_pos) -> uint32 diagonal; set hits (string_id, string_pos, text_pos, 0) -> uint64
// (diagonal | string_id << 32), the uint2 (diagonal, string_id)
template <bool SET>
__global__ void __launch_bounds__(256)
qgram_diagonal_kernel(const void* __restrict__ hits, const uint32_t n, const uint32_t interval, void* __restrict__ keys)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        if (SET)
        {
            const uint4 h = ((const uint4*)hits)[i];
            ((uint64_t*)keys)[i] = (uint64_t)snap_diagonal( h.z - h.y, interval ) | ((uint64_t)h.x << 32);
        }
        else
        {
            const uint2 h = ((const uint2*)hits)[i];
            ((uint32_t*)keys)[i] = snap_diagonal( h.y - h.x, interval );
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static nvbio_status check_qgram_params(const uint32_t q, const uint32_t ss, const uint32_t qlut)
{
    NVB_REQUIRE( ss >= 1 && ss <= 8, "symbol_size must be in [1, 8]" );
    NVB_REQUIRE( q >= 1 && (uint64_t)q * ss <= 64, "q must be >= 1 with q * symbol_size <= 64" );
    NVB_REQUIRE( qlut <= q, "qlut must be <= q" );
    NVB_REQUIRE( (uint64_t)qlut * ss <= 28, "qlut * symbol_size must be <= 28" );
    return NVBIO_OK;
}

static nvbio_status check_text_bits(const uint32_t bits)
{
    NVB_REQUIRE( bits == 2 || bits == 4 || bits == 8, "text_bits must be 2, 4 or 8" );
    return NVBIO_OK;
}

// sort (q-gram, coordinate) pairs stably over [0, q * ss), run-length encode them and build slots and the LUT; hands qgrams, slots,
// index and lut to a new handle.  keys / vals hold n entries (the unsorted pairs); V is uint32 or uint64 (a uint2 coordinate).
template <typename V>
static nvbio_status finish_index(BuildBuffers& bufs, const int device, const uint32_t q, const uint32_t ss, const uint32_t qlut, const uint32_t is_set,
                                 const uint32_t n, uint64_t* keys, V* vals, hipStream_t s, nvbio_qgram_index_t* out)
{
    NVB_ALLOC( skeys, uint64_t, n );
    NVB_ALLOC( index, V, n );
    NVB_ALLOC( qgrams, uint64_t, n );
    NVB_ALLOC( counts, uint32_t, n );
    NVB_ALLOC( d_runs, uint64_t, 1 );
    uint64_t n_unique = 0;
    if (n)
    {
        size_t a = 0, b = 0;
        NVB_HIP( rocprim::radix_sort_pairs( nullptr, a, keys, skeys, vals, index, (size_t)n, 0u, q * ss, s ) );
        NVB_HIP( rocprim::run_length_encode( nullptr, b, skeys, (size_t)n, qgrams, counts, d_runs, s ) );
        NVB_ALLOC( temp, uint8_t, a > b ? a : b );
        NVB_HIP( rocprim::radix_sort_pairs( temp, a, keys, skeys, vals, index, (size_t)n, 0u, q * ss, s ) );
        NVB_HIP( rocprim::run_length_encode( temp, b, skeys, (size_t)n, qgrams, counts, d_runs, s ) );
        NVB_HIP( hipMemcpyAsync( &n_unique, d_runs, 8, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp );
    }
    bufs.release( keys ); bufs.release( vals ); bufs.release( skeys );
    // slots = exclusive scan of the counts (n_unique + 1 entries)
    NVB_ALLOC( slots, uint32_t, n_unique + 1u );
    NVB_HIP( hipMemsetAsync( slots, 0, 4, s ) );
    if (n_unique)
    {
        size_t a = 0;
        NVB_HIP( rocprim::inclusive_scan( nullptr, a, counts, slots + 1, (size_t)n_unique, rocprim::plus<uint32_t>(), s ) );
        NVB_ALLOC( temp, uint8_t, a );
        NVB_HIP( rocprim::inclusive_scan( temp, a, counts, slots + 1, (size_t)n_unique, rocprim::plus<uint32_t>(), s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp );
    }
    bufs.release( counts ); bufs.release( d_runs );
    uint64_t lut_size = 0;
    uint32_t* lut = nullptr;
    const uint32_t qls = (q - qlut) * ss;
    if (qlut)
    {
        lut_size = 1ull << (qlut * ss);
        lut = bufs.alloc<uint32_t>( lut_size + 1u );
        if (!lut) { set_error( "q-gram index build: out of device memory (lut, %llu bytes)", (unsigned long long)(4u * (lut_size + 1u)) ); return NVBIO_ERR_NOMEM; }
        NVB_CHECK( NVB_LAUNCH( qgram_lut_kernel, dim3( grid_for( lut_size + 1u ) ), dim3(256), s, (const uint64_t*)qgrams, (uint32_t)n_unique, qls,
                               lut_size, lut ) );
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    nvbio_qgram_index_s* h = new (std::nothrow) nvbio_qgram_index_s();
    if (!h) { set_error( "out of host memory" ); return NVBIO_ERR_NOMEM; }
    h->device = device; h->q = q; h->symbol_size = ss; h->qlut = qlut; h->is_set = is_set;
    h->n_qgrams = n; h->n_unique = (uint32_t)n_unique;
    h->qgrams = qgrams; h->slots = slots; h->index = index; h->lut = lut; h->lut_size = lut_size;
    h->bytes = 8ull * n + sizeof(V) * (uint64_t)n + 4ull * (n_unique + 1u) + (lut ? 4ull * (lut_size + 1u) : 0u);
    bufs.forget( qgrams ); bufs.forget( slots ); bufs.forget( index );
    if (lut) bufs.forget( lut );
    *out = h;
    return NVBIO_OK;
}

// the argument checks both set builds share: a plain string set and a seed interval
static nvbio_status check_plain_set(const nvbio_string_set* set, const uint32_t seed_interval)
{
    NVB_REQUIRE( seed_interval >= 1, "seed_interval must be >= 1" );
    NVB_REQUIRE( set->seeds_per_string == 0 && set->seed_intervals_dev == nullptr, "the q-gram set index takes plain string sets, not seed enumerations" );
    NVB_REQUIRE( set->n == 0 || set->symbols_dev != nullptr, "symbols_dev is NULL" );
    NVB_REQUIRE( !(set->offsets_are_ranges && set->offsets_dev == nullptr), "offsets_are_ranges without offsets_dev" );
    NVB_REQUIRE( set->n < 0xFFFFFFFFu, "more than 2^32 - 2 strings" );
    return NVBIO_OK;
}

// the seeds of a plain set in string-major order: n of them, their q-grams in keys and their (string_id, string_pos) in coords,
// both buffers of `bufs`
static nvbio_status enumerate_set_seeds(BuildBuffers& bufs, const nvbio_string_set* set, const uint32_t q, const uint32_t symbol_size,
                                        const uint32_t seed_interval, hipStream_t s, uint32_t& n_out, uint64_t*& keys_out, uint64_t*& coords_out)
{
    QGramSet qs{ set->symbols_dev, set->offsets_dev, set->offsets_are_ranges, set->fixed_len, set->stride, set->n };
    NVB_ALLOC( cnt, uint64_t, set->n + 1u );
    NVB_ALLOC( first, uint64_t, set->n + 1u );
    uint64_t total = 0;
    NVB_HIP( hipMemsetAsync( first, 0, 8, s ) );
    if (set->n)
    {
        NVB_CHECK( NVB_LAUNCH( qgram_seed_count_kernel, dim3( grid_for( set->n ) ), dim3(256), s, qs, q, seed_interval, cnt ) );
        size_t a = 0;
        NVB_HIP( rocprim::inclusive_scan( nullptr, a, cnt, first + 1, (size_t)set->n, rocprim::plus<uint64_t>(), s ) );
        NVB_ALLOC( temp, uint8_t, a );
        NVB_HIP( rocprim::inclusive_scan( temp, a, cnt, first + 1, (size_t)set->n, rocprim::plus<uint64_t>(), s ) );
        NVB_HIP( hipMemcpyAsync( &total, first + set->n, 8, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp );
    }
    bufs.release( cnt );
    NVB_REQUIRE( total < 0xFFFFFFFFull, "the set has 2^32 - 1 seeds or more" );
    const uint32_t n = (uint32_t)total;
    NVB_ALLOC( keys, uint64_t, n );
    NVB_ALLOC( coords, uint64_t, n );
    if (n)
    {
        NVB_CHECK( with_value( SymbolBits(), set->symbol_bits, [&](auto BITS)
        {
            return NVB_LAUNCH( qgram_seed_enumerate_kernel<BITS>, dim3( grid_for( n ) ), dim3(256), s, qs, q, symbol_size, seed_interval,
                               (const uint64_t*)first, n, keys, (uint2*)coords );
        }, bad_symbol_bits ) );
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    bufs.release( first );
    n_out = n; keys_out = keys; coords_out = coords;
    return NVBIO_OK;
}

static QGramView view_of(const nvbio_qgram_index_s* h)
{
    QGramView v;
    v.qgrams = h->qgrams; v.slots = h->slots; v.lut = h->lut; v.lut_size = h->lut_size; v.n_unique = h->n_unique;
    v.qls = (h->q - h->qlut) * h->symbol_size;
    return v;
}

// the caller's temp of rank: the inclusive scan's temporaries
static uint64_t rank_cub_bytes(const uint32_t n)
{
    size_t a = 0;
    rocprim::transform_iterator<const uint2*, QGramRangeSize, uint64_t> sizes( (const uint2*)nullptr, QGramRangeSize() );
    (void)rocprim::inclusive_scan( nullptr, a, sizes, (uint64_t*)nullptr, (size_t)(n ? n : 1u), rocprim::plus<uint64_t>() );
    return a;
}

// the caller's temp of merge: two key buffers, the run count, the sort's and the encoder's temporaries
struct MergeTemp
{
    void* keys; void* sorted; uint64_t* runs; uint8_t* cub; uint64_t cub_bytes;
    template <typename K> static uint64_t cub_need(const uint32_t n)
    {
        size_t a = 0, b = 0;
        const size_t m = n ? n : 1u;
        (void)rocprim::radix_sort_keys( nullptr, a, (const K*)nullptr, (K*)nullptr, m, 0u, 8u * sizeof(K) );
        (void)rocprim::run_length_encode( nullptr, b, (const K*)nullptr, m, (K*)nullptr, (uint32_t*)nullptr, (uint64_t*)nullptr );
        return a > b ? a : b;
    }
    void carve(ScratchLayout& c, const bool set, const uint32_t n)
    {
        const uint64_t w = set ? 8u : 4u;
        keys = c.take<uint8_t>( w * n ); sorted = c.take<uint8_t>( w * n ); runs = c.take<uint64_t>( 1 );
        cub_bytes = set ? cub_need<uint64_t>( n ) : cub_need<uint32_t>( n );
        cub = c.take<uint8_t>( cub_bytes );
    }
};

// the caller's temp of a sorted generate_qgrams: the unsorted pairs and the sort's temporaries
struct GenerateTemp
{
    uint64_t* keys; uint32_t* pos; uint8_t* cub; uint64_t cub_bytes;
    void carve(ScratchLayout& c, const uint32_t n)
    {
        keys = c.take<uint64_t>( n ); pos = c.take<uint32_t>( n );
        size_t a = 0;
        (void)rocprim::radix_sort_pairs( nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         (size_t)(n ? n : 1u), 0u, 64u );
        cub_bytes = a;
        cub = c.take<uint8_t>( cub_bytes );
    }
};

} // namespace nvbio_amd

#include "qgroup_inl.h"                                   // the q-group index: its build, lookup and entry points

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_qgram_index_build(int device, const void* text_dev, uint32_t text_bits, uint32_t length, uint32_t q, uint32_t symbol_size,
                                     uint32_t qlut, nvbio_qgram_index_t* out, void* stream)
{
    NVB_REQUIRE( out != nullptr, "out is NULL" );
    *out = nullptr;
    NVB_CHECK( check_text_bits( text_bits ) );
    NVB_CHECK( check_qgram_params( q, symbol_size, qlut ) );
    NVB_REQUIRE( length == 0 || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( length < 0xFFFFFFFFu, "length must be below 2^32 - 1" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    BuildBuffers bufs( "q-gram index build" );
    NVB_ALLOC( keys, uint64_t, length );
    NVB_ALLOC( pos, uint32_t, length );
    if (length)
    {
        NVB_CHECK( with_value( SymbolBits(), text_bits, [&](auto BITS)
        {
            return NVB_LAUNCH( qgram_extract_kernel<BITS>, dim3( grid_for( length ) ), dim3(256), s, text_dev, length, q, symbol_size, 0u,
                               length, keys, pos );
        }, bad_symbol_bits ) );
    }
    return finish_index<uint32_t>( bufs, device, q, symbol_size, qlut, 0u, length, keys, pos, s, out );
}

nvbio_status nvbio_qgram_set_index_build(int device, const nvbio_string_set* set, uint32_t q, uint32_t symbol_size, uint32_t seed_interval,
                                         uint32_t qlut, nvbio_qgram_index_t* out, void* stream)
{
    NVB_REQUIRE( out != nullptr && set != nullptr, "NULL argument" );
    *out = nullptr;
    NVB_CHECK( check_text_bits( set->symbol_bits ) );
    NVB_CHECK( check_qgram_params( q, symbol_size, qlut ) );
    NVB_CHECK( check_plain_set( set, seed_interval ) );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    BuildBuffers bufs( "q-gram index build" );
    uint32_t n = 0; uint64_t* keys = nullptr; uint64_t* coords = nullptr;
    NVB_CHECK( enumerate_set_seeds( bufs, set, q, symbol_size, seed_interval, s, n, keys, coords ) );
    return finish_index<uint64_t>( bufs, device, q, symbol_size, qlut, 1u, n, keys, coords, s, out );
}

nvbio_status nvbio_qgram_index_destroy(nvbio_qgram_index_t index)
{
    if (!index) return NVBIO_OK;
    int prev = -1;
    if (hipGetDevice( &prev ) != hipSuccess) prev = -1;
    (void)hipSetDevice( index->device );
    (void)hipFree( index->qgrams ); (void)hipFree( index->slots ); (void)hipFree( index->index );
    if (index->lut) (void)hipFree( index->lut );
    if (index->table) (void)hipFree( index->table );
    if (prev >= 0) (void)hipSetDevice( prev );
    delete index;
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_index_get_view(nvbio_qgram_index_t index, nvbio_qgram_index_view* view)
{
    NVB_REQUIRE( index && view, "NULL argument" );
    view->q = index->q; view->symbol_size = index->symbol_size; view->qlut = index->qlut; view->is_set = index->is_set;
    view->n_qgrams = index->n_qgrams; view->n_unique = index->n_unique; view->lut_size = index->lut_size; view->device = index->device;
    view->qgrams_dev = index->qgrams; view->slots_dev = index->slots; view->index_dev = index->index; view->lut_dev = index->lut;
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_index_device_bytes(nvbio_qgram_index_t index, uint64_t* bytes)
{
    NVB_REQUIRE( index && bytes, "NULL argument" );
    *bytes = index->bytes;
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_index_export(nvbio_qgram_index_t index, uint64_t* qgrams_out_dev, uint32_t* slots_out_dev, void* index_out_dev,
                                      uint32_t* lut_out_dev, void* stream)
{
    NVB_REQUIRE( index != nullptr, "index is NULL" );
    NVB_REQUIRE( !index->is_group, "a q-group index is exported by nvbio_qgroup_index_export" );
    DeviceGuard g( index->device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t w = index->is_set ? 8u : 4u;
    if (qgrams_out_dev && index->n_unique) NVB_HIP( hipMemcpyAsync( qgrams_out_dev, index->qgrams, 8ull * index->n_unique, hipMemcpyDeviceToDevice, s ) );
    if (slots_out_dev) NVB_HIP( hipMemcpyAsync( slots_out_dev, index->slots, 4ull * (index->n_unique + 1u), hipMemcpyDeviceToDevice, s ) );
    if (index_out_dev && index->n_qgrams) NVB_HIP( hipMemcpyAsync( index_out_dev, index->index, w * index->n_qgrams, hipMemcpyDeviceToDevice, s ) );
    if (lut_out_dev && index->lut) NVB_HIP( hipMemcpyAsync( lut_out_dev, index->lut, 4ull * (index->lut_size + 1u), hipMemcpyDeviceToDevice, s ) );
    return NVBIO_OK;
}

nvbio_status nvbio_generate_qgrams_temp_bytes(uint32_t n, int sort, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    if (!sort) { *bytes = 0; return NVBIO_OK; }
    GenerateTemp t; ScratchLayout c( nullptr, scratch_check_enabled() ); t.carve( c, n );
    *bytes = c.bytes();
    return NVBIO_OK;
}

nvbio_status nvbio_generate_qgrams(int device, uint32_t q, uint32_t symbol_size, const void* text_dev, uint32_t text_bits, uint32_t text_len,
                                   uint32_t first_pos, uint32_t n, uint64_t* qgrams_dev, uint32_t* indices_dev, int sort,
                                   void* temp_dev, uint64_t temp_bytes, void* stream)
{
    NVB_CHECK( check_text_bits( text_bits ) );
    NVB_CHECK( check_qgram_params( q, symbol_size, 0u ) );
    NVB_REQUIRE( (uint64_t)first_pos + n <= 0xFFFFFFFFull, "first_pos + n must not exceed 2^32 - 1" );
    if (n == 0) return NVBIO_OK;
    NVB_REQUIRE( qgrams_dev != nullptr, "qgrams_dev is NULL" );
    NVB_REQUIRE( text_len == 0 || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( !sort || (indices_dev != nullptr && temp_dev != nullptr), "a sorted call needs indices_dev and temp_dev" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    uint64_t* keys = qgrams_dev; uint32_t* pos = indices_dev;
    GenerateTemp T;
    ScratchBlock temp;
    if (sort)
    {
        NVB_CHECK( temp.alloc_layout( "qgram_generate", s, "generate_qgrams: out of device memory", [&](ScratchLayout& c) { T.carve( c, n ); },
                                      temp_dev, temp_bytes, "nvbio_generate_qgrams_temp_bytes" ) );
        keys = T.keys; pos = T.pos;
    }
    NVB_CHECK( with_value( SymbolBits(), text_bits, [&](auto BITS)
    {
        return NVB_LAUNCH( qgram_extract_kernel<BITS>, dim3( grid_for( n ) ), dim3(256), s, text_dev, text_len, q, symbol_size, first_pos, n,
                           keys, pos );
    }, bad_symbol_bits ) );
    if (sort)
    {
        size_t bytes = T.cub_bytes;
        NVB_HIP( rocprim::radix_sort_pairs( T.cub, bytes, T.keys, qgrams_dev, T.pos, indices_dev, (size_t)n, 0u, q * symbol_size, s ) );
    }
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_ranges(nvbio_qgram_index_t index, const uint64_t* qgrams_dev, uint32_t n, nvbio_uint2* ranges_dev, void* stream)
{
    NVB_REQUIRE( index != nullptr, "index is NULL" );
    if (n == 0) return NVBIO_OK;
    NVB_REQUIRE( qgrams_dev && ranges_dev, "NULL device pointer" );
    DeviceGuard g( index->device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    return launch_ranges( index, qgrams_dev, n, (uint2*)ranges_dev, (hipStream_t)stream );
}

nvbio_status nvbio_qgram_filter_temp_bytes(uint32_t n_queries, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    ScratchLayout c( nullptr, scratch_check_enabled() ); c.take<uint8_t>( rank_cub_bytes( n_queries ) );
    *bytes = c.bytes();
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_filter_rank(nvbio_qgram_index_t index, const uint64_t* qgrams_dev, uint32_t n, nvbio_uint2* ranges_dev, uint64_t* slots_dev,
                                     void* temp_dev, uint64_t temp_bytes, uint64_t* n_hits, void* stream)
{
    NVB_REQUIRE( index && n_hits, "NULL argument" );
    *n_hits = 0;
    if (n == 0) return NVBIO_OK;
    NVB_REQUIRE( qgrams_dev && ranges_dev && slots_dev && temp_dev, "NULL device pointer" );
    DeviceGuard g( index->device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cub_bytes = rank_cub_bytes( n );
    uint8_t* cub = nullptr;
    ScratchBlock temp;
    NVB_CHECK( temp.alloc_layout( "qgram_filter_rank", s, "q-gram filter rank: out of device memory", [&](ScratchLayout& c) { cub = c.take<uint8_t>( cub_bytes ); },
                                  temp_dev, temp_bytes, "nvbio_qgram_filter_temp_bytes" ) );
    NVB_CHECK( launch_ranges( index, qgrams_dev, n, (uint2*)ranges_dev, s ) );
    rocprim::transform_iterator<const uint2*, QGramRangeSize, uint64_t> sizes( (const uint2*)ranges_dev, QGramRangeSize() );
    size_t bytes = cub_bytes;
    NVB_HIP( rocprim::inclusive_scan( cub, bytes, sizes, slots_dev, (size_t)n, rocprim::plus<uint64_t>(), s ) );
    NVB_HIP( hipMemcpyAsync( n_hits, slots_dev + (n - 1u), 8, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_filter_locate(nvbio_qgram_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev, const uint32_t* indices_dev,
                                       uint32_t n, uint64_t begin, uint64_t end, void* hits_dev, void* stream)
{
    NVB_REQUIRE( index != nullptr, "index is NULL" );
    if (end <= begin) return NVBIO_OK;
    NVB_REQUIRE( ranges_dev && slots_dev && indices_dev && hits_dev, "NULL device pointer" );
    NVB_REQUIRE( n > 0, "locate over an empty filter" );
    DeviceGuard g( index->device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    uint64_t n_hits = 0;                                      // an output past the last hit would read past the ranges
    NVB_HIP( hipMemcpyAsync( &n_hits, slots_dev + (n - 1u), 8, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    NVB_REQUIRE( end <= n_hits, "end is past the last hit (slots[n - 1])" );
    const dim3 grid( expand_grid( begin, end ) ), block( 256 );
    if (index->is_set) NVB_CHECK( NVB_LAUNCH( qgram_locate_kernel<true>, grid, block, s, (const void*)index->index, (const uint2*)ranges_dev,
                                              slots_dev, indices_dev, n, begin, end, hits_dev ) );
    else               NVB_CHECK( NVB_LAUNCH( qgram_locate_kernel<false>, grid, block, s, (const void*)index->index, (const uint2*)ranges_dev,
                                              slots_dev, indices_dev, n, begin, end, hits_dev ) );
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_filter_merge_temp_bytes(int is_set, uint32_t n_hits, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    MergeTemp t; ScratchLayout c( nullptr, scratch_check_enabled() ); t.carve( c, is_set != 0, n_hits );
    *bytes = c.bytes();
    return NVBIO_OK;
}

nvbio_status nvbio_qgram_filter_merge(int device, int is_set, uint32_t interval, const void* hits_dev, uint32_t n_hits, void* merged_dev,
                                      uint32_t* counts_dev, uint32_t* n_merged, void* temp_dev, uint64_t temp_bytes, void* stream)
{
    NVB_REQUIRE( n_merged != nullptr, "n_merged is NULL" );
    *n_merged = 0;
    NVB_REQUIRE( interval >= 1, "interval must be >= 1" );
    if (n_hits == 0) return NVBIO_OK;
    NVB_REQUIRE( hits_dev && merged_dev && counts_dev && temp_dev, "NULL device pointer" );
    const bool set = is_set != 0;
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    MergeTemp T;
    ScratchBlock temp;
    NVB_CHECK( temp.alloc_layout( "qgram_filter_merge", s, "q-gram filter merge: out of device memory", [&](ScratchLayout& c) { T.carve( c, set, n_hits ); },
                                  temp_dev, temp_bytes, "nvbio_qgram_filter_merge_temp_bytes" ) );
    const dim3 grid( grid_for( n_hits ) ), block( 256 );
    size_t a = T.cub_bytes, b = T.cub_bytes;
    if (set)
    {
        NVB_CHECK( NVB_LAUNCH( qgram_diagonal_kernel<true>, grid, block, s, hits_dev, n_hits, interval, T.keys ) );
        NVB_HIP( rocprim::radix_sort_keys( T.cub, a, (const uint64_t*)T.keys, (uint64_t*)T.sorted, (size_t)n_hits, 0u, 64u, s ) );
        NVB_HIP( rocprim::run_length_encode( T.cub, b, (const uint64_t*)T.sorted, (size_t)n_hits, (uint64_t*)merged_dev, counts_dev, T.runs, s ) );
    }
    else
    {
        NVB_CHECK( NVB_LAUNCH( qgram_diagonal_kernel<false>, grid, block, s, hits_dev, n_hits, interval, T.keys ) );
        NVB_HIP( rocprim::radix_sort_keys( T.cub, a, (const uint32_t*)T.keys, (uint32_t*)T.sorted, (size_t)n_hits, 0u, 32u, s ) );
        NVB_HIP( rocprim::run_length_encode( T.cub, b, (const uint32_t*)T.sorted, (size_t)n_hits, (uint32_t*)merged_dev, counts_dev, T.runs, s ) );
    }
    uint64_t runs = 0;
    NVB_HIP( hipMemcpyAsync( &runs, T.runs, 8, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    *n_merged = (uint32_t)runs;
    return NVBIO_OK;
}

} // extern "C"
