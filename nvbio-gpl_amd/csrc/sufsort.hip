// sufsort.hip -- the suffix sort and the BWT of a string set for gfx950 (the single-string forms are in fm_build.hip).
//
// Reference behaviour reproduced (file:line relative to the reference tree):
//   cuda::suffix_sort( string_set, ... )               nvbio/sufsort/sufsort.h, sufsort_inl.h:70-135
//   cuda::bwt<SYMBOL_SIZE, BIG_ENDIAN>( string_set )    sufsort_inl.h:535-560 (the "dollar" block first)
//   string_set_bwt_functor (255 in front of a string)   sufsort_priv.h:881-904
//   SetSuffixFlattener (the global suffix index)        sufsort_priv.h
//
// Semantics.  A suffix is (pos, string_id), 0 <= pos <= len; pos == len is the empty suffix.  Suffixes compare by raw symbol value,
// a proper prefix first (the implicit '$' below every symbol), and suffixes equal up to and including their ends by ascending
// string_id -- so the N empty suffixes come first, in string order.  bwt[r] is the symbol in front of the r-th suffix, 255 when
// pos == 0.  NVBIO_SUFSORT_NO_EMPTY_SUFFIXES drops the empty suffixes from every output.  The global index of a suffix is pos plus
// the exclusive sum of (len + 1), or of len under the flag, over the strings before it.
//
// Departures from the reference:
//   method   the reference sorts ALL suffixes once per 14-symbol word, least significant word first: ceil( (max_len + 1) / 14 ) full
//            sorts.  Here the most significant word is sorted once and only the suffixes that still tie are refined (below).  The
//            order is the same: both are stable from the string-major initial order.
//   symbols  8-bit symbols sort by their whole byte (the reference's set sorter is instantiated for 2, 4 and 8 bits and does the same).
//
// The sorter, most significant word first.  With W symbols per word (29 of 2 bits, 15 of 4, 7 of 8):
//   round 0  every suffix gets a 64-bit key: its first W symbols, zero past its end, above a count field that holds min( W, the
//            symbols it has left ).  The count sits in the low bits, so a suffix that ends inside the word sorts before one that
//            goes on with symbol 0.  One stable rocPRIM radix sort of (key, global index) from string-major order.
//   classify a suffix whose count is below W has ended: equal ended suffixes are already in string order.  A suffix whose key no
//            neighbour shares is final.  The others -- full words that tie -- are selected into the unresolved list, with the slot
//            of their segment's head as segment id.
//   round k  over the unresolved list only: word k of every suffix; a stable sort by word, then a stable sort by segment (two radix
//            passes over the list); the values go back to the slots; new heads are flagged where (segment, word) changes; what
//            still ties with a full word is compacted and goes on.  A suffix of length L is final after floor( L / W ) + 1 rounds.
//   emit     one pass turns the sorted global indices into (pos, string_id), the global index and the BWT byte.
//
// MI355X shape.  Key extraction is one lane per suffix: consecutive suffixes of a string are neighbouring lanes and read the same two
// or three words (unaligned funnel read: three guarded 32-bit loads, one 96-bit shift), for all three packings.  In round 0 a
// workgroup bounds the strings of its 256 suffixes once (expand_ranges, range_expand.h) and each lane searches those few entries;
// later rounds and the emit pass see suffixes in sorted order, so a lane divides (fixed-length sets) or reads the string id round 0
// stored for its suffix (ragged sets: 4 bytes per suffix more).  Every grid-stride loop runs on a 64-bit index: n may come within one
// grid of 2^32.
// Sorts, scans, reductions and selects are rocPRIM.  Storage: BuildBuffers / NVB_ALLOC only (no ScratchBlock site); every buffer is
// freed before the call returns.
// Registers (gfx950 code object, -Rpass-analysis=kernel-resource-usage): VGPRs count 10, first word 21-22, next word 19, first heads,
// place and compact 14, emit 16, cum 7; private_segment_fixed_size = 0 (no scratch, no private arrays) for every one.
// Measured (scripts/bench_sufsort.py): the refinement wins where ties are rare and loses to the reference's eight full
// sorts on reads at 30x coverage and on all-A text, where nearly every suffix with a full word left ties.
#include "range_expand.h"
#include "build_prims.h"

namespace nvbio_amd {
namespace {

// string i of a plain set: its first symbol and its length
struct SufSet
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

// the key word of a packing: W symbols above a count field of CNT bits
template <int BITS> struct SufWord;
template <> struct SufWord<2> { static constexpr uint32_t W = 29u, CNT = 5u; };
template <> struct SufWord<4> { static constexpr uint32_t W = 15u, CNT = 4u; };
template <> struct SufWord<8> { static constexpr uint32_t W = 7u,  CNT = 3u; };

// the key of `count` (<= W) symbols from symbol `first` of the stream on: the symbols big-endian, zero padded to W, above the count
template <int BITS>
__device__ __forceinline__ uint64_t suffix_word(const void* symbols, const uint64_t first, const uint32_t count)
{
    constexpr uint32_t W = SufWord<BITS>::W, CNT = SufWord<BITS>::CNT;
    if (count == 0u) return 0ull;
    const uint32_t* words;
    uint32_t sh, last;                                               // bit offset in words[0]; index of the last word that holds a symbol
    if (BITS == 8)
    {
        const uint64_t a = (uint64_t)symbols + first;                // bytes: the aligned words around them, byte-swapped to big-endian
        words = (const uint32_t*)(a & ~3ull);
        sh    = 8u * (uint32_t)(a & 3u);
        last  = (uint32_t)(((a + count - 1u) >> 2) - (a >> 2));
    }
    else
    {
        constexpr uint32_t LOG = (BITS == 2) ? 4u : 3u;
        words = (const uint32_t*)symbols + (first >> LOG);
        sh    = BITS * (uint32_t)(first & ((1u << LOG) - 1u));
        last  = (uint32_t)(((first + count - 1u) >> LOG) - (first >> LOG));
    }
    uint32_t w0 = words[0];
    uint32_t w1 = last >= 1u ? words[1] : 0u;
    uint32_t w2 = last >= 2u ? words[2] : 0u;
    if (BITS == 8) { w0 = __builtin_bswap32( w0 ); w1 = __builtin_bswap32( w1 ); w2 = __builtin_bswap32( w2 ); }
    const uint64_t hi = ((uint64_t)w0 << 32) | w1;
    uint64_t v = sh ? ((hi << sh) | (uint64_t)(w2 >> (32u - sh))) : hi;
    v &= ~0ull << (64u - BITS * count);
    return ((v >> (64u - BITS * W)) << CNT) | count;
}

// global suffix index -> (string, position).  first[n + 1]: first[i] = the suffixes of the strings before i.  A set of equal
// lengths divides; a ragged one reads the string of each suffix from string_of[n_suffixes], which round 0 writes while it has it.
struct SufMap
{
    const uint64_t* first;
    const uint32_t* string_of;                                       // ragged sets only, else NULL
    uint32_t        per_string;                                      // suffixes per string of a fixed-length set, else 0
    __device__ __forceinline__ void locate(const uint32_t g, uint32_t& sid, uint32_t& pos) const
    {
        if (per_string) { sid = g / per_string; pos = g - sid * per_string; }
        else            { sid = string_of[g];   pos = g - (uint32_t)first[sid]; }
    }
};

// cnt[i] = the suffixes of string i: len + extra (extra = 1 with the empty suffix)
__global__ void __launch_bounds__(256)
sufsort_count_kernel(const SufSet set, const uint32_t extra, uint64_t* __restrict__ cnt)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < set.n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        uint32_t begin, len;
        set.bounds( (uint32_t)i, begin, len );
        cnt[i] = (uint64_t)len + extra;
    }
}

// round 0: keys[g] = word 0 of suffix g, over the shared expansion in tiles of 256 suffixes (`first` read as an inclusive scan has
// the empty range 0 in front, so suffix g falls into range sid + 1 and base = first[sid]); string_of[g] = sid for a ragged set
template <int BITS>
__global__ void __launch_bounds__(256)
sufsort_first_word_kernel(const SufSet set, const uint64_t* __restrict__ first, const uint32_t n_suffixes, uint64_t* __restrict__ keys,
                          uint32_t* __restrict__ string_of /* may be NULL */)
{
    expand_ranges<256u>( first, set.n + 1u, 0u, n_suffixes, [&](const uint64_t g, const uint32_t i, const uint64_t base)
    {
        const uint32_t pos = (uint32_t)(g - base);
        uint32_t begin, len;
        set.bounds( i - 1u, begin, len );
        const uint32_t left = len - pos;
        keys[g] = suffix_word<BITS>( set.symbols, (uint64_t)begin + pos, left < SufWord<BITS>::W ? left : SufWord<BITS>::W );
        if (string_of) string_of[g] = i - 1u;
    } );
}

// round k: word[j] = word k of unresolved suffix gid[j], sg[j] = its segment above its global index
template <int BITS>
__global__ void __launch_bounds__(256)
sufsort_next_word_kernel(const SufSet set, const SufMap map, const uint32_t* __restrict__ gid, const uint32_t* __restrict__ seg, const uint32_t m,
                         const uint32_t k, uint64_t* __restrict__ word, uint64_t* __restrict__ sg)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint32_t g = gid[j];
        uint32_t sid, pos, begin, len;
        map.locate( g, sid, pos );
        set.bounds( sid, begin, len );
        const uint64_t p    = (uint64_t)pos + (uint64_t)k * SufWord<BITS>::W;
        const uint64_t left = p < len ? len - p : 0u;
        word[j] = suffix_word<BITS>( set.symbols, (uint64_t)begin + p, left < SufWord<BITS>::W ? (uint32_t)left : SufWord<BITS>::W );
        sg[j]   = ((uint64_t)seg[j] << 32) | g;
    }
}

// a full word (count == W) that a neighbour shares: the suffix is still tied
struct FirstUnresolved
{
    const uint64_t* keys; uint32_t n, cnt_mask, w;
    __device__ __forceinline__ bool operator()(const uint32_t s) const
    {
        const uint64_t k = keys[s];
        if (((uint32_t)k & cnt_mask) != w) return false;
        return (s > 0u && keys[s - 1u] == k) || (s + 1u < n && keys[s + 1u] == k);
    }
};

// the unresolved list after round 0: the global index of each listed slot, and head[j] = its slot where a segment starts, else 0
__global__ void __launch_bounds__(256)
sufsort_first_heads_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ slot, const uint32_t m,
                           uint32_t* __restrict__ gid, uint32_t* __restrict__ head)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint32_t s = slot[j];
        gid[j]  = sorted[s];
        head[j] = (j == 0u || keys[s] != keys[slot[j - 1u]]) ? s : 0u;
    }
}

// after the two passes of round k: the values back into their slots, head[j] = the slot where (segment, word) changes, else 0
__global__ void __launch_bounds__(256)
sufsort_place_kernel(const uint64_t* __restrict__ word, const uint64_t* __restrict__ sg, const uint32_t* __restrict__ slot, const uint32_t m,
                     uint32_t* __restrict__ sorted, uint32_t* __restrict__ head)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t v = sg[j];
        const uint32_t s = slot[j];
        sorted[s] = (uint32_t)v;
        head[j]   = (j == 0u || (sg[j - 1u] >> 32) != (v >> 32) || word[j - 1u] != word[j]) ? s : 0u;
    }
}

// seg (max-scanned heads) holds the head slot of every listed suffix: tied = a full word in a segment of more than one
struct StillUnresolved
{
    const uint64_t* word; const uint32_t* seg; const uint32_t* slot; uint32_t m, cnt_mask, w;
    __device__ __forceinline__ bool operator()(const uint32_t j) const
    {
        if (((uint32_t)word[j] & cnt_mask) != w) return false;
        const bool head      = seg[j] == slot[j];
        const bool next_head = j + 1u >= m || seg[j + 1u] == slot[j + 1u];
        return !(head && next_head);
    }
};

// the unresolved list of the next round
__global__ void __launch_bounds__(256)
sufsort_compact_kernel(const uint32_t* __restrict__ sel, const uint32_t m2, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ seg,
                       const uint64_t* __restrict__ sg, uint32_t* __restrict__ slot2, uint32_t* __restrict__ seg2, uint32_t* __restrict__ gid2)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m2; j += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint32_t i = sel[j];
        slot2[j] = slot[i]; seg2[j] = seg[i]; gid2[j] = (uint32_t)sg[i];
    }
}

// the outputs of sorted suffix r (any may be NULL): (pos, string_id), the global index, the string id alone, the symbol in front (255
// in front of a string)
template <int BITS>
__global__ void __launch_bounds__(256)
sufsort_emit_kernel(const SufSet set, const SufMap map, const uint32_t* __restrict__ sorted, const uint32_t n, uint2* __restrict__ suffixes,
                    uint32_t* __restrict__ global, uint32_t* __restrict__ string_ids, uint8_t* __restrict__ bwt)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint32_t g = sorted[r];
        uint32_t sid, pos;
        map.locate( g, sid, pos );
        if (suffixes) suffixes[r] = make_uint2( pos, sid );
        if (global)   global[r]   = g;
        if (string_ids) string_ids[r] = sid;
        if (bwt)
        {
            uint32_t begin, len;
            set.bounds( sid, begin, len );
            SymbolReader<BITS> rd( set.symbols );
            bwt[r] = pos ? (uint8_t)rd.get( begin + pos - 1u ) : (uint8_t)255u;
        }
    }
}

// cum[i] = first[i + 1]: the suffixes of the strings up to and including i (the reference's cum_lengths)
__global__ void __launch_bounds__(256)
sufsort_cum_kernel(const uint64_t* __restrict__ first, const uint32_t n_strings, uint32_t* __restrict__ cum)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_strings; i += (uint64_t)gridDim.x * blockDim.x)
        cum[i] = (uint32_t)first[i + 1u];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

static nvbio_status check_set(const nvbio_string_set* set, const uint32_t flags)
{
    NVB_REQUIRE( set != nullptr, "set is NULL" );
    NVB_REQUIRE( (flags & ~(uint32_t)NVBIO_SUFSORT_NO_EMPTY_SUFFIXES) == 0, "unknown flag" );
    NVB_REQUIRE( set->symbol_bits == 2 || set->symbol_bits == 4 || set->symbol_bits == 8, "symbol_bits must be 2, 4 or 8" );
    NVB_REQUIRE( set->seeds_per_string == 0 && set->seed_intervals_dev == nullptr, "the suffix sort takes plain string sets, not seed enumerations" );
    NVB_REQUIRE( set->n == 0 || set->symbols_dev != nullptr, "symbols_dev is NULL" );
    NVB_REQUIRE( !(set->offsets_are_ranges && set->offsets_dev == nullptr), "offsets_are_ranges without offsets_dev" );
    NVB_REQUIRE( set->n < 0xFFFFFFFFu, "more than 2^32 - 2 strings" );
    return NVBIO_OK;
}

static SufSet set_of(const nvbio_string_set* set)
{
    return SufSet{ set->symbols_dev, set->offsets_dev, set->offsets_are_ranges, set->fixed_len, set->stride, set->n };
}

struct MaxU64
{
    __device__ __host__ __forceinline__ uint64_t operator()(const uint64_t a, const uint64_t b) const { return a > b ? a : b; }
};

// first[n + 1] = the scan of the strings' suffix counts (first[0] = 0), a buffer of `bufs`; n_suffixes = first[n]; max_count = the
// largest count.  NVBIO_ERR_INVALID when the suffixes, the empty ones included, do not fit 32-bit indices.
static nvbio_status count_suffixes(BuildBuffers& bufs, const nvbio_string_set* set, const uint32_t flags, hipStream_t s, uint64_t*& first_out,
                                   uint32_t& n_suffixes, uint32_t& max_count)
{
    const uint32_t extra = (flags & NVBIO_SUFSORT_NO_EMPTY_SUFFIXES) ? 0u : 1u;
    NVB_ALLOC( first, uint64_t, set->n + 1ull );
    NVB_HIP( hipMemsetAsync( first, 0, 8, s ) );
    uint64_t total = 0, longest = 0;
    if (set->n)
    {
        NVB_ALLOC( cnt, uint64_t, set->n );
        NVB_ALLOC( d_max, uint64_t, 1 );
        NVB_CHECK( NVB_LAUNCH( sufsort_count_kernel, dim3( grid_for( set->n ) ), dim3(256), s, set_of( set ), extra, cnt ) );
        size_t a = 0, b = 0;
        NVB_HIP( rocprim::inclusive_scan( nullptr, a, cnt, first + 1, (size_t)set->n, rocprim::plus<uint64_t>(), s ) );
        NVB_HIP( rocprim::reduce( nullptr, b, cnt, d_max, (uint64_t)0, (size_t)set->n, MaxU64(), s ) );
        NVB_ALLOC( temp, uint8_t, a > b ? a : b );
        NVB_HIP( rocprim::inclusive_scan( temp, a, cnt, first + 1, (size_t)set->n, rocprim::plus<uint64_t>(), s ) );
        NVB_HIP( rocprim::reduce( temp, b, cnt, d_max, (uint64_t)0, (size_t)set->n, MaxU64(), s ) );
        NVB_HIP( hipMemcpyAsync( &total, first + set->n, 8, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipMemcpyAsync( &longest, d_max, 8, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( temp ); bufs.release( d_max ); bufs.release( cnt );
    }
    NVB_REQUIRE( total + (extra ? 0u : set->n) < 0xFFFFFFFFull, "the set has 2^32 - 1 suffixes or more (the sum of len + 1)" );
    first_out = first; n_suffixes = (uint32_t)total; max_count = (uint32_t)longest;
    return NVBIO_OK;
}

// the position of the highest set bit of x, plus one (0 for 0)
static uint32_t bit_length(const uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll( x ) : 0u; }

// sorted[n] = the global indices of the n suffixes in sorted order, a buffer of `bufs`; round 0 fills string_of (a ragged set's map)
template <int BITS>
static nvbio_status sort_set_suffixes(BuildBuffers& bufs, const SufSet set, const SufMap map, uint32_t* string_of, const uint32_t n, const uint32_t max_count,
                                      const uint32_t extra, hipStream_t s, nvbio_sufsort_stats& st, uint32_t*& sorted_out)
{
    constexpr uint32_t W = SufWord<BITS>::W, CNT = SufWord<BITS>::CNT, KEY_BITS = BITS * W + CNT, CNT_MASK = (1u << CNT) - 1u;
    const dim3 block( 256 );
    NVB_ALLOC( sorted, uint32_t, n );
    sorted_out = sorted;
    // a suffix of length L is final after floor( L / W ) + 1 rounds; the longest has max_count - extra symbols
    const uint32_t max_rounds = (max_count - extra) / W + 1u;

    // ---- round 0: every suffix, by its first word -------------------------------------------------
    uint64_t m = 0;
    uint32_t* slot = nullptr;
    uint32_t* gid  = nullptr;
    uint32_t* seg  = nullptr;
    {
        NVB_ALLOC( keys,  uint64_t, n );
        NVB_ALLOC( skeys, uint64_t, n );
        NVB_CHECK( NVB_LAUNCH( sufsort_first_word_kernel<BITS>, dim3( grid_for( n ) ), block, s, set, map.first, n, keys, string_of ) );
        NVB_CHECK( sort_pairs( keys, skeys, rocprim::counting_iterator<uint32_t>( 0 ), sorted, (size_t)n, 0u, KEY_BITS, bufs, s ) );
        bufs.release( keys );
        st.rounds = 1; st.sorted_per_round[0] = n;
        NVB_ALLOC( slot0, uint32_t, n );
        FirstUnresolved pred{ skeys, n, CNT_MASK, W };
        NVB_CHECK( select_indices( n, pred, slot0, &m, bufs, s ) );
        if (m)
        {
            NVB_ALLOC( slot_, uint32_t, m );
            NVB_ALLOC( gid_,  uint32_t, m );
            NVB_ALLOC( seg_,  uint32_t, m );
            slot = slot_; gid = gid_; seg = seg_;
            NVB_HIP( hipMemcpyAsync( slot, slot0, 4ull * m, hipMemcpyDeviceToDevice, s ) );
            NVB_CHECK( NVB_LAUNCH( sufsort_first_heads_kernel, dim3( grid_for( m ) ), block, s, (const uint64_t*)skeys, (const uint32_t*)sorted,
                                   (const uint32_t*)slot, (uint32_t)m, gid, seg ) );
            NVB_CHECK( scan_max_inplace( seg, m, bufs, s ) );
        }
        NVB_HIP( hipStreamSynchronize( s ) );
        bufs.release( slot0 ); bufs.release( skeys );
    }
    if (m == 0) return NVBIO_OK;

    // ---- rounds k > 0: the unresolved list only ---------------------------------------------------
    const uint64_t m0 = m;
    const uint32_t seg_bits = bit_length( n - 1u );
    NVB_ALLOC( word,  uint64_t, m0 );
    NVB_ALLOC( word2, uint64_t, m0 );
    NVB_ALLOC( sg,    uint64_t, m0 );
    NVB_ALLOC( sg2,   uint64_t, m0 );
    NVB_ALLOC( head,  uint32_t, m0 );
    NVB_ALLOC( sel,   uint32_t, m0 );
    NVB_ALLOC( slot2, uint32_t, m0 );
    NVB_ALLOC( gid2,  uint32_t, m0 );
    for (uint32_t k = 1; m > 0; ++k)
    {
        if (k >= max_rounds)
        {
            set_error( "set suffix sort: %llu suffixes still tie after %u rounds (at most %u expected)", (unsigned long long)m, k, max_rounds );
            return NVBIO_ERR_HIP;
        }
        const uint32_t mm = (uint32_t)m;
        const dim3 grid( grid_for( mm ) );
        if (k < 16u) st.sorted_per_round[k] = mm;
        st.rounds = k + 1u;
        NVB_CHECK( NVB_LAUNCH( sufsort_next_word_kernel<BITS>, grid, block, s, set, map, (const uint32_t*)gid, (const uint32_t*)seg, mm, k, word, sg ) );
        NVB_CHECK( sort_pairs( word, word2, sg, sg2, (size_t)mm, 0u, KEY_BITS, bufs, s ) );                // by word ...
        NVB_CHECK( sort_pairs( sg2, sg, word2, word, (size_t)mm, 32u, 32u + seg_bits, bufs, s ) );         // ... then, stably, by segment
        NVB_CHECK( NVB_LAUNCH( sufsort_place_kernel, grid, block, s, (const uint64_t*)word, (const uint64_t*)sg, (const uint32_t*)slot, mm, sorted, head ) );
        NVB_CHECK( scan_max_inplace( head, mm, bufs, s ) );
        uint64_t m2 = 0;
        StillUnresolved pred{ word, head, slot, mm, CNT_MASK, W };
        NVB_CHECK( select_indices( mm, pred, sel, &m2, bufs, s ) );
        if (m2)
        {
            NVB_CHECK( NVB_LAUNCH( sufsort_compact_kernel, dim3( grid_for( m2 ) ), block, s, (const uint32_t*)sel, (uint32_t)m2, (const uint32_t*)slot,
                                   (const uint32_t*)head, (const uint64_t*)sg, slot2, seg, gid2 ) );
            uint32_t* t = slot; slot = slot2; slot2 = t;
            t = gid; gid = gid2; gid2 = t;
        }
        m = m2;
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    bufs.release( word ); bufs.release( word2 ); bufs.release( sg ); bufs.release( sg2 ); bufs.release( head ); bufs.release( sel );
    bufs.release( slot ); bufs.release( slot2 ); bufs.release( gid ); bufs.release( gid2 ); bufs.release( seg );
    return NVBIO_OK;
}

// what a call writes per sorted suffix (any may be NULL), and per string
struct SetSortOutputs
{
    uint2*    suffixes    = nullptr;     // (pos, string_id)
    uint32_t* global      = nullptr;
    uint32_t* string_ids  = nullptr;
    uint8_t*  bwt         = nullptr;
    uint32_t* cum_lengths = nullptr;     // n strings: the inclusive scan of their suffix counts
};

// count, check the capacity, sort, emit
static nvbio_status set_sort_impl(const nvbio_string_set* set, const uint32_t flags, const SetSortOutputs out, const uint64_t capacity,
                                  uint32_t* n_out, nvbio_sufsort_stats* stats, hipStream_t s)
{
    BuildBuffers bufs( "set suffix sort" );
    const uint32_t extra = (flags & NVBIO_SUFSORT_NO_EMPTY_SUFFIXES) ? 0u : 1u;
    uint64_t* first = nullptr;
    uint32_t n = 0, max_count = 0;
    NVB_CHECK( count_suffixes( bufs, set, flags, s, first, n, max_count ) );
    *n_out = n;
    nvbio_sufsort_stats st;
    memset( &st, 0, sizeof(st) );
    st.n_suffixes = n;
    st.symbols_per_word = set->symbol_bits == 2 ? SufWord<2>::W : set->symbol_bits == 4 ? SufWord<4>::W : SufWord<8>::W;
    if (capacity < n)
    {
        set_error( "invalid argument: capacity %llu too small: the set has %u suffixes", (unsigned long long)capacity, n );
        return NVBIO_ERR_INVALID;
    }
    if (out.cum_lengths && set->n)
        NVB_CHECK( NVB_LAUNCH( sufsort_cum_kernel, dim3( grid_for( set->n ) ), dim3(256), s, (const uint64_t*)first, set->n, out.cum_lengths ) );
    if (n)
    {
        NVB_REQUIRE( out.suffixes || out.global || out.string_ids || out.bwt, "NULL output pointer" );
        const SufSet ss = set_of( set );
        const bool ragged = set->offsets_dev && set->offsets_are_ranges;
        uint32_t* string_of = nullptr;
        if (ragged) { NVB_ALLOC( string_of_, uint32_t, n ); string_of = string_of_; }
        const SufMap map{ first, string_of, ragged ? 0u : set->fixed_len + extra };
        uint32_t* sorted = nullptr;
        NVB_CHECK( with_value( SymbolBits(), (int)set->symbol_bits, [&](auto BITS)
        {
            NVB_CHECK( sort_set_suffixes<BITS>( bufs, ss, map, string_of, n, max_count, extra, s, st, sorted ) );
            return NVB_LAUNCH( sufsort_emit_kernel<BITS>, dim3( grid_for( n ) ), dim3(256), s, ss, map, (const uint32_t*)sorted, n, out.suffixes,
                               out.global, out.string_ids, out.bwt );
        }, bad_symbol_bits ) );
    }
    NVB_HIP( hipStreamSynchronize( s ) );
    st.peak_bytes = bufs.peak;
    if (stats) *stats = st;
    return NVBIO_OK;
}

} // anonymous namespace
} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_set_suffix_count(int device, const nvbio_string_set* set, uint32_t flags, uint32_t* n_suffixes, void* stream)
{
    NVB_REQUIRE( n_suffixes != nullptr, "n_suffixes is NULL" );
    *n_suffixes = 0;
    NVB_CHECK( check_set( set, flags ) );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    BuildBuffers bufs( "set suffix count" );
    uint64_t* first = nullptr;
    uint32_t max_count = 0;
    return count_suffixes( bufs, set, flags, (hipStream_t)stream, first, *n_suffixes, max_count );
}

nvbio_status nvbio_set_suffix_sort(int device, const nvbio_string_set* set, uint32_t flags, nvbio_uint2* suffixes_dev, uint32_t* global_dev,
                                   uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream)
{
    NVB_REQUIRE( n_suffixes != nullptr, "n_suffixes is NULL" );
    *n_suffixes = 0;
    NVB_CHECK( check_set( set, flags ) );
    NVB_REQUIRE( capacity == 0 || suffixes_dev != nullptr, "suffixes_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    SetSortOutputs out; out.suffixes = (uint2*)suffixes_dev; out.global = global_dev;
    return set_sort_impl( set, flags, out, capacity, n_suffixes, stats, (hipStream_t)stream );
}

nvbio_status nvbio_set_suffix_sort_flat(int device, const nvbio_string_set* set, uint32_t flags, uint32_t* suffix_array_dev, uint32_t* string_ids_dev,
                                        uint32_t* cum_lengths_dev, uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream)
{
    NVB_REQUIRE( n_suffixes != nullptr, "n_suffixes is NULL" );
    *n_suffixes = 0;
    NVB_CHECK( check_set( set, flags ) );
    NVB_REQUIRE( capacity == 0 || suffix_array_dev != nullptr, "suffix_array_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    SetSortOutputs out; out.global = suffix_array_dev; out.string_ids = string_ids_dev; out.cum_lengths = cum_lengths_dev;
    return set_sort_impl( set, flags, out, capacity, n_suffixes, stats, (hipStream_t)stream );
}

nvbio_status nvbio_set_bwt(int device, const nvbio_string_set* set, uint32_t flags, uint8_t* bwt_dev, nvbio_uint2* suffixes_dev,
                           uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream)
{
    NVB_REQUIRE( n_suffixes != nullptr, "n_suffixes is NULL" );
    *n_suffixes = 0;
    NVB_CHECK( check_set( set, flags ) );
    NVB_REQUIRE( capacity == 0 || bwt_dev != nullptr, "bwt_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    SetSortOutputs out; out.bwt = bwt_dev; out.suffixes = (uint2*)suffixes_dev;
    return set_sort_impl( set, flags, out, capacity, n_suffixes, stats, (hipStream_t)stream );
}

} // extern "C"
