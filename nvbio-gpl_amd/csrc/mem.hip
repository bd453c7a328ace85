// mem.hip -- SMEM seeding for gfx950: the bidirectional MEM filter over a forward and a reverse FM-index, behind the C ABI.
//
// Reference behaviour reproduced (file:line relative to the reference tree):
//   extend_forward                        nvbio/fmindex/bidir_inl.h           (with the sentinel: see "Departures")
//   right_kmems / right_mem_functor       nvbio/fmindex/mem_inl.h:474-627
//   split_mem_functor (the #else branch)  mem_inl.h:629-770
//   left_mem_functor                      mem_inl.h:776-857
//   discard_ranges_kernel                 mem_inl.h:971-1040
//   MEMFilter<device_tag>::rank / locate  mem_inl.h:1303-1528
//
// The passes, in the reference's order and with its internal entry order (the second discard's containment test depends on it):
//   right   per read, x = 0; while x < len: x = max( right_kmems( x ), x + 1 ).  Each x-group in emit order (largest end first,
//           the first entry flagged).  A group's ends lie in (x, next x], so a read has at most len candidates: they go to a region
//           of len entries at the read's own symbol offset, with no count pass and no atomics.
//   left    per candidate: backward steps on the forward index until an N, the read start or a size below min_intv.
//   discard per read and group, in entry order: keep iff span.x < leftmost && span >= min_span && occurrences <= max_intv; the
//           left-most marker moves only for kept MEMs (the device filter; the host find_kmems moves it also for a MEM its handler
//           drops for max_intv -- tests/test_mem_oracle.py shows the kept sets are equal: a MEM dropped for max_intv is followed in
//           its group only by MEMs that begin further left, or that begin at the same place and have no fewer occurrences).
//   split   (split_len < 0xFFFFFFFF) per kept MEM with span >= split_len and occurrences <= split_width: right_kmems from its
//           midpoint with min_intv = occurrences + 1 replaces it; then left and discard again.  The first discard keeps the order.
//   output  per read ascending (span begin, span end), reads by string id; slots = inclusive scan (uint64) of the range sizes.
//
// Departures from the reference (reference defects, not reproduced):
//   sentinel    extend_forward counts the suffixes that start with P.d, d < c, but not the one suffix P$ (P a suffix of the text):
//               the reference's forward ranges are one row low from the first step on (sizes are right).  Here a range is the
//               exact SA interval of its span: the '$' row of the reverse index inside the reverse range adds one.
//   span begin  MEMRange::span() and lookup_ssa_results mask the begin with 0xFF: spans are wrong from 256 symbols on.  Not here.
//   order       the reference reverses a group only when the next one starts (the last group of each read stays as it is); the
//               order here is the one its comments intend, ascending (span begin, span end) inside a read (stable).
//   capacity    the reference drops MEMs silently when its per-thread 1024-entry arrays or its 256 x n_reads arena fill up.
//               Nothing is dropped here: a short caller buffer fails with NVBIO_ERR_INVALID and a message naming the size needed.
//
// MI355X shape: every pass is a chain of dependent 32-byte record gathers (as the seed pass).  One lane per read (right, discard,
// output) or per entry (left, split); no per-lane arrays (a runtime-indexed private array would live in scratch): each lane keeps its
// current (f_range, r_range, prev_range) in registers and writes every pushed range straight to global memory.  One forward step of
// the reverse index is one rank4 at two rows -- one record, or two when the rows fall in different 64-symbol blocks.
// Working storage is the caller's temp (nvbio_mem_filter_temp_bytes), two ScratchBlocks: see MemTemp.
#include "fm_device.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

constexpr uint32_t MEM_FLAG    = 1u << 31;     // MEMRange::GROUP_FLAG
constexpr uint32_t MEM_MAX_LEN = 65535u;       // the span packs two 16-bit coordinates

// errors a kernel reports through err[0] (bits)
constexpr uint32_t MEM_ERR_LONG  = 1u;         // a read longer than MEM_MAX_LEN, or offsets that go backwards
constexpr uint32_t MEM_ERR_BOUND = 2u;         // an internal bound was violated (a bug: nothing was written past it)

struct MemReads
{
    const void*     symbols;
    const uint32_t* offsets;     // NULL: read i = [i * stride, + fixed_len)
    uint32_t        ranges;      // offsets hold n + 1 begin/end pairs (ragged); else n starts and fixed_len
    uint32_t        fixed_len;
    uint32_t        stride;
    uint32_t        n;
};

// read i: its first symbol, its length and the first entry of its candidate region (regions are laid out as the symbols)
__device__ __forceinline__ void read_bounds(const MemReads& q, const uint32_t i, uint32_t& begin, uint32_t& len, uint32_t& region)
{
    if (q.offsets && q.ranges) { begin = q.offsets[i]; len = q.offsets[i + 1] - begin; region = begin - q.offsets[0]; }
    else                       { begin = q.offsets ? q.offsets[i] : i * q.stride; len = q.fixed_len; region = i * q.fixed_len; }
}

__device__ __forceinline__ uint32_t span_begin(const uint4 m) { return m.w & 0xFFFFu; }
__device__ __forceinline__ uint32_t span_end(const uint4 m)   { return m.w >> 16; }

// counts of the four symbols in BWT rows [0, k] of f (rank4, fmindex_inl.h:96-123) from a record already loaded when `have`
__device__ __forceinline__ void rank4_row(const DevIndex& f, const uint32_t k, uint32_t out[4], uint32_t& blk, bool& have, uint4& b, uint4& o,
                                          uint32_t& nrec)
{
    uint32_t kt, dummy;
    if (!resolve_row( f, k, 0u, &kt, &dummy ))
    {
        const bool end = (k == f.length);
        out[0] = end ? count_of( f, 0 ) : 0u; out[1] = end ? count_of( f, 1 ) : 0u;
        out[2] = end ? count_of( f, 2 ) : 0u; out[3] = end ? count_of( f, 3 ) : 0u;
        return;
    }
    const uint32_t kb = kt >> 6;
    if (!have || kb != blk) { b = f.rec[2u * kb]; o = f.rec[2u * kb + 1u]; blk = kb; have = true; ++nrec; }
    const uint4 c = count4_in_block( b, kt & 63u );
    out[0] = o.x + c.x; out[1] = o.y + c.y; out[2] = o.z + c.z; out[3] = o.w + c.w;
}

// extend_forward (bidir_inl.h): the forward range of P -> that of Pc, through the reverse range of P^R -> that of cP^R.
// Suffixes of the text that start with P and sort before Pc: P$ (iff the '$' row of the reverse index, its primary, lies in
// the reverse range) and P.d for d < c.
__device__ __forceinline__ void extend_forward(const DevIndex& r, uint32_t& fx, uint32_t& fy, uint32_t& rx, uint32_t& ry, const uint32_t c,
                                               uint32_t& nrec)
{
    uint32_t lo[4], hi[4], blk = 0; bool have = false; uint4 b, o;
    rank4_row( r, rx - 1u, lo, blk, have, b, o, nrec );
    rank4_row( r, ry,      hi, blk, have, b, o, nrec );
    uint32_t before = (rx <= r.primary && r.primary <= ry) ? 1u : 0u;
    before += (c > 0u ? hi[0] - lo[0] : 0u) + (c > 1u ? hi[1] - lo[1] : 0u) + (c > 2u ? hi[2] - lo[2] : 0u);
    const uint32_t lc = pick4( lo[0], lo[1], lo[2], lo[3], c ), hc = pick4( hi[0], hi[1], hi[2], hi[3], c );
    const uint32_t base = L2_of( r, c );
    rx = base + lc + 1u;
    ry = base + hc;
    fx = fx + before;
    fy = fx + (hc - lc) - 1u;
}

// right_kmems (mem_inl.h:474-551) from x: the ranges of [x, e) for every e at which the SA interval size changes, written to
// out[n_out..] in emit order (largest end first, that one flagged).  WRITE = false only counts.  Returns the largest end, or x
// when there is none.  Entries past `cap` are counted, not written, and flag `bound`.
template <int BITS, bool WRITE>
__device__ __forceinline__ uint32_t right_kmems(const DevIndex& f, const DevIndex& r, SymbolReader<BITS>& rd, const uint32_t begin, const uint32_t len,
                                                const uint32_t sid, const uint32_t x, const uint32_t min_intv,
                                                uint4* __restrict__ out, uint32_t& n_out, const uint32_t cap, bool& bound, uint32_t& nrec)
{
    uint32_t fx = 0u, fy = f.length, rx = 0u, ry = r.length;
    uint32_t px = fx, py = fy;                                  // prev_range
    uint32_t ld = 0u, last_end = x;                             // size - 1 of the last pushed range, and its end
    const uint32_t g0 = n_out;
    auto push = [&](const uint32_t e) {
        if (WRITE) { if (n_out < cap) out[n_out] = make_uint4( px, py, sid, x | (e << 16) ); else bound = true; }
        ++n_out; ld = py - px; last_end = e;
    };
    uint32_t i;
    for (i = x; i < len; ++i)
    {
        const uint32_t c = rd.get( begin + i );
        if (c > 3u) { px = fx; py = fy; break; }                // an N: no match
        extend_forward( r, fx, fy, rx, ry, c, nrec );
        if (1u + fy - fx < min_intv) break;                     // the range became too small
        if (fy - fx != py - px)
        {
            if (i > x) push( i );                               // (not the empty span)
            px = fx; py = fy;
        }
    }
    if (n_out != g0 && ld != py - px) push( i );
    if (n_out == g0) return x;
    if (WRITE)
    {
        const uint32_t e = n_out < cap ? n_out : cap;           // reverse the group in place: emit order
        for (uint32_t a = g0, z = e - 1u; a < z; ++a, --z) { const uint4 t = out[a]; out[a] = out[z]; out[z] = t; }
        if (g0 < cap) out[g0].z |= MEM_FLAG;
    }
    return last_end;
}

__device__ __forceinline__ void add_records(uint64_t* __restrict__ records, const uint32_t nrec)
{
    uint64_t v = nrec;                                           // one atomic per wave
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor( v, d );
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd( (unsigned long long*)records, (unsigned long long)v );
}

// right pass: one lane per read, candidates at cand[region..], their number in cnt[i]
template <int BITS>
__global__ void __launch_bounds__(256)
mem_right_kernel(const DevIndex f, const DevIndex r, const MemReads q, const uint32_t total, const uint32_t min_intv,
                 uint4* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t* __restrict__ err, uint64_t* __restrict__ records)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t iters = (q.n + stride - 1u) / stride;        // uniform trip count: every lane reaches the wave reduction
    uint32_t nrec = 0;
    for (uint32_t t = 0, i = i0; t < iters; ++t, i += stride)
    {
        if (i >= q.n) continue;
        uint32_t begin, len, region;
        read_bounds( q, i, begin, len, region );
        if (len > MEM_MAX_LEN || (uint64_t)region + len > total) { atomicOr( err, MEM_ERR_LONG ); cnt[i] = 0u; continue; }
        SymbolReader<BITS> rd( q.symbols );
        uint32_t k = 0; bool bound = false;
        for (uint32_t x = 0; x < len;)
        {
            const uint32_t y = right_kmems<BITS, true>( f, r, rd, begin, len, i, x, min_intv, cand + region, k, len, bound, nrec );
            x = y > x + 1u ? y : x + 1u;
        }
        if (bound) { atomicOr( err, MEM_ERR_BOUND ); k = len; }
        cnt[i] = k;
    }
    add_records( records, nrec );
}

// compaction of the candidates: dense[off[i]..] = cand[region(i)..+cnt[i])
__global__ void __launch_bounds__(256)
mem_gather_kernel(const MemReads q, const uint4* __restrict__ cand, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                  uint4* __restrict__ dense)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < q.n; i += gridDim.x * blockDim.x)
    {
        uint32_t begin, len, region;
        read_bounds( q, i, begin, len, region );
        const uint32_t n = cnt[i], o = off[i];
        for (uint32_t k = 0; k < n; ++k) dense[o + k] = cand[region + k];
    }
}

// left pass (left_mem_functor, mem_inl.h:776-857): one lane per entry of mems[0, n)
template <int BITS>
__global__ void __launch_bounds__(256)
mem_left_kernel(const DevIndex f, const MemReads q, uint4* __restrict__ mems, const uint32_t n, const uint32_t min_intv, uint64_t* __restrict__ records)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t iters = (n + stride - 1u) / stride;
    uint32_t nrec = 0;
    for (uint32_t t = 0, e = blockIdx.x * blockDim.x + threadIdx.x; t < iters; ++t, e += stride)
    {
        if (e >= n) continue;
        const uint4 m = mems[e];
        uint32_t begin, len, region;
        read_bounds( q, m.z & ~MEM_FLAG, begin, len, region );
        SymbolReader<BITS> rd( q.symbols );
        uint32_t x = m.x, y = m.y;
        int32_t l;
        for (l = (int32_t)span_begin( m ) - 1; l >= 0; --l)
        {
            const uint32_t c = rd.get( begin + (uint32_t)l );
            if (c > 3u) break;
            uint32_t nx = x, ny = y;
            search_step<true>( f, nx, ny, c, nrec );
            if (1u + ny - nx < min_intv) break;
            x = nx; y = ny;
        }
        mems[e] = make_uint4( x, y, m.z, (uint32_t)(l + 1) | (span_end( m ) << 16) );
    }
    add_records( records, nrec );
}

// discard (discard_ranges_kernel without the reversal, mem_inl.h:971-1040): per read, mems[base(i), + n(i)) compacted in place,
// the kept count to kept[i].  base(i) = off[i] (after the right pass) or soff[off[i]] (after the split); n(i) likewise.
__global__ void __launch_bounds__(256)
mem_discard_kernel(const uint32_t n_reads, const uint32_t* __restrict__ off, const uint32_t* __restrict__ soff, uint4* __restrict__ mems,
                   const uint32_t max_intv, const uint32_t min_span, uint32_t* __restrict__ kept)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += gridDim.x * blockDim.x)
    {
        const uint32_t b = soff ? soff[off[i]] : off[i];
        const uint32_t e = soff ? soff[off[i + 1]] : off[i + 1];
        uint32_t leftmost = 0xFFFFFFFFu, o = b;
        for (uint32_t j = b; j < e; ++j)
        {
            uint4 m = mems[j];
            if (m.z & MEM_FLAG) leftmost = 0xFFFFFFFFu;
            const uint32_t sb = span_begin( m ), se = span_end( m );
            if (sb < leftmost && se - sb >= min_span && 1u + m.y - m.x <= max_intv)
            {
                if (leftmost == 0xFFFFFFFFu) m.z |= MEM_FLAG;
                mems[o++] = m;
                leftmost = sb;
            }
        }
        kept[i] = o - b;
    }
}

// split (split_mem_functor, #else branch): one lane per entry of dense[0, n) that the first discard kept.  COUNT: scnt[k] = the
// entries it becomes (0 if not kept, 1 if not split, else the size of its right_kmems group from the midpoint); !COUNT: writes them
// to arena[soff[k], soff[k+1]).
template <int BITS, bool COUNT>
__global__ void __launch_bounds__(256)
mem_split_kernel(const DevIndex f, const DevIndex r, const MemReads q, const uint4* __restrict__ dense, const uint32_t n,
                 const uint32_t* __restrict__ off, const uint32_t* __restrict__ kept, const uint32_t split_len, const uint32_t split_width,
                 uint32_t* __restrict__ scnt, const uint32_t* __restrict__ soff, uint4* __restrict__ arena, const uint32_t arena_cap,
                 uint32_t* __restrict__ err, uint64_t* __restrict__ records)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t iters = (n + stride - 1u) / stride;
    uint32_t nrec = 0;
    for (uint32_t t = 0, k = blockIdx.x * blockDim.x + threadIdx.x; t < iters; ++t, k += stride)
    {
        if (k >= n) continue;
        const uint4 m = dense[k];
        const uint32_t sid = m.z & ~MEM_FLAG;
        if (k - off[sid] >= kept[sid]) { if (COUNT) scnt[k] = 0u; continue; }
        const uint32_t sb = span_begin( m ), se = span_end( m ), occ = 1u + m.y - m.x;
        if (se - sb >= split_len && occ <= split_width)
        {
            uint32_t begin, len, region;
            read_bounds( q, sid, begin, len, region );
            SymbolReader<BITS> rd( q.symbols );
            uint32_t w = COUNT ? 0u : soff[k]; bool bound = false;
            const uint32_t end = COUNT ? 0u : soff[k + 1];
            right_kmems<BITS, !COUNT>( f, r, rd, begin, len, sid, (sb + se) / 2u, occ + 1u, arena, w, end < arena_cap ? end : arena_cap, bound, nrec );
            if (COUNT) scnt[k] = w;
            else if (bound || w != end) atomicOr( err, MEM_ERR_BOUND );
        }
        else if (COUNT) scnt[k] = 1u;
        else if (soff[k] < arena_cap) arena[soff[k]] = m;
        else atomicOr( err, MEM_ERR_BOUND );
    }
    add_records( records, nrec );
}

// output: ranges[first[i]..] = the kept entries of read i, in ascending (span begin, span end) (stable insertion sort)
__global__ void __launch_bounds__(256)
mem_output_kernel(const uint32_t n_reads, const uint32_t* __restrict__ off, const uint32_t* __restrict__ soff, const uint4* __restrict__ mems,
                  const uint32_t* __restrict__ first, uint4* __restrict__ ranges)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += gridDim.x * blockDim.x)
    {
        const uint32_t b = soff ? soff[off[i]] : off[i];
        const uint32_t o = first[i], n = first[i + 1] - o;
        for (uint32_t j = 0; j < n; ++j)
        {
            const uint4 m = mems[b + j];
            const uint32_t key = (span_begin( m ) << 16) | span_end( m );
            uint32_t p = j;
            for (; p > 0u; --p)
            {
                const uint4 prev = ranges[o + p - 1u];
                if (((span_begin( prev ) << 16) | span_end( prev )) <= key) break;
                ranges[o + p] = prev;
            }
            ranges[o + p] = m;
        }
    }
}

// locate (MEMFilter::locate, mem_inl.h:1463-1505): hits[h - begin] = (text position, string id, span begin, span end) of the global
// MEM index h, over the shared expansion (locate_ranges, fm_device.h)
__global__ void __launch_bounds__(256)
mem_locate_kernel(const DevIndex f, const uint4* __restrict__ ranges, const uint64_t* __restrict__ slots, const uint32_t n_ranges,
                  const uint64_t begin, const uint64_t end, uint4* __restrict__ hits)
{
    uint4 m = make_uint4( 0, 0, 0, 0 );                          // the MEM of the index this lane is walking to
    locate_ranges( f, slots, n_ranges, begin, end,
        [&](const uint64_t h, const uint32_t i, const uint64_t base, uint32_t& row) {
            m = ranges[i];
            row = m.x + (uint32_t)(h - base);
            return true;
        },
        [&](const uint64_t h, const uint32_t pos) { hits[h - begin] = make_uint4( pos, m.z & ~MEM_FLAG, span_begin( m ), span_end( m ) ); } );
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static nvbio_status mem_reads(const nvbio_string_set* s, MemReads* q)
{
    NVB_REQUIRE( s != nullptr, "reads is NULL" );
    NVB_REQUIRE( s->symbol_bits == 2 || s->symbol_bits == 4 || s->symbol_bits == 8, "symbol_bits must be 2, 4 or 8" );
    NVB_REQUIRE( s->seeds_per_string == 0 && s->seed_intervals_dev == nullptr, "the MEM filter takes plain string sets, not seed enumerations" );
    NVB_REQUIRE( s->n == 0 || s->symbols_dev != nullptr, "symbols_dev is NULL" );
    NVB_REQUIRE( !(s->offsets_are_ranges && s->offsets_dev == nullptr), "offsets_are_ranges without offsets_dev" );
    NVB_REQUIRE( s->offsets_are_ranges || s->fixed_len <= MEM_MAX_LEN, "reads longer than 65535 symbols are not supported" );
    q->symbols = s->symbols_dev; q->offsets = s->offsets_dev; q->ranges = s->offsets_are_ranges;
    q->fixed_len = s->fixed_len; q->stride = s->stride; q->n = s->n;
    return NVBIO_OK;
}

// the number of symbols the candidate regions cover: n x fixed_len, or offsets[n] - offsets[0] of a ragged set (read from the device)
static nvbio_status mem_total(const MemReads& q, hipStream_t s, uint64_t* total)
{
    *total = 0;
    if (q.n == 0) return NVBIO_OK;
    if (!(q.offsets && q.ranges)) { *total = (uint64_t)q.n * q.fixed_len; }
    else
    {
        uint32_t a = 0, b = 0;
        NVB_HIP( hipMemcpyAsync( &a, q.offsets, 4, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipMemcpyAsync( &b, q.offsets + q.n, 4, hipMemcpyDeviceToHost, s ) );
        NVB_HIP( hipStreamSynchronize( s ) );
        NVB_REQUIRE( b >= a, "ragged read offsets go backwards" );
        *total = b - a;
    }
    NVB_REQUIRE( *total < 0xFFFFFFFFull, "more than 2^32 - 2 read symbols in one call" );
    return NVBIO_OK;
}

// the caller's temp, two blocks: the head -- per-read counters, per-candidate scan arrays, the dense candidates -- and, from the
// head's rounded end, the arena -- the candidate regions (reused as the split arena, of `cap` >= total entries) and the scans'
// hipcub temporaries.  A larger split arena lays out the arena again and leaves the head alone: the head is live by then, the arena is not.
struct MemTemp
{
    uint32_t* cnt;   uint32_t* off;  uint32_t* kept; uint32_t* first_tmp;
    uint32_t* scnt;  uint32_t* soff; uint32_t* misc;   // misc: [0] error bits, [2..3] records (uint64)
    uint4*    dense; uint4* cand;    uint8_t* cub;   uint64_t cub_bytes;

    static uint64_t cub_need(uint64_t n_items)
    {
        size_t a = 0, b = 0;
        const int n = (int)(n_items ? n_items : 1);
        (void)hipcub::DeviceScan::InclusiveSum( nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, n );
        hipcub::TransformInputIterator<uint64_t, RangeSize, const uint4*> sizes( (const uint4*)nullptr, RangeSize() );
        (void)hipcub::DeviceScan::InclusiveSum( nullptr, b, sizes, (uint64_t*)nullptr, n );
        return a > b ? a : b;
    }
    void head(ScratchLayout& c, uint32_t n, uint64_t total)
    {
        cnt  = c.take<uint32_t>( n + 1u ); off = c.take<uint32_t>( n + 1u ); kept = c.take<uint32_t>( n + 1u );
        first_tmp = c.take<uint32_t>( n + 1u );
        scnt = c.take<uint32_t>( total + 1u ); soff = c.take<uint32_t>( total + 1u );
        misc = c.take<uint32_t>( 8 );
        dense = c.take<uint4>( total );
    }
    void arena(ScratchLayout& c, uint32_t n, uint64_t cap)
    {
        cand = c.take<uint4>( cap );
        cub_bytes = cub_need( (cap > n ? cap : n) + 1u );
        cub = c.take<uint8_t>( cub_bytes );
    }
    static uint64_t head_end(uint32_t n, uint64_t total)     // where the arena starts, before rounding
    {
        MemTemp t; ScratchLayout c( nullptr, scratch_check_enabled() ); t.head( c, n, total );
        return c.end();
    }
};

// exclusive scan of in[0, n) into out[0, n] (out[n] = the total)
static nvbio_status scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, MemTemp& T, hipStream_t s)
{
    NVB_HIP( hipMemsetAsync( out, 0, 4, s ) );
    if (n == 0) return NVBIO_OK;
    size_t bytes = T.cub_bytes;
    NVB_HIP( hipcub::DeviceScan::InclusiveSum( T.cub, bytes, in, out + 1, (int)n, s ) );
    return NVBIO_OK;
}

static nvbio_status read_u32(const uint32_t* p, uint32_t* v, hipStream_t s)
{
    NVB_HIP( hipMemcpyAsync( v, p, 4, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    return NVBIO_OK;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_mem_filter_temp_bytes(const nvbio_string_set* reads, const nvbio_mem_params* params, uint64_t* bytes, void* stream)
{
    NVB_REQUIRE( reads && params && bytes, "NULL argument" );
    MemReads q; NVB_CHECK( mem_reads( reads, &q ) );
    uint64_t total = 0; NVB_CHECK( mem_total( q, (hipStream_t)stream, &total ) );
    MemTemp t; ScratchLayout arena( nullptr, scratch_check_enabled() ); t.arena( arena, q.n, total );
    ScratchLayout both; both.take<uint8_t>( MemTemp::head_end( q.n, total ) ); both.take<uint8_t>( arena.end() );   // as nvbio_mem_filter_rank adopts them
    *bytes = both.bytes();
    return NVBIO_OK;
}

nvbio_status nvbio_mem_filter_rank(nvbio_fm_index_t f_index, nvbio_fm_index_t r_index, const nvbio_string_set* reads,
                                   const nvbio_mem_params* params, nvbio_mem_range* ranges_dev, uint32_t max_ranges,
                                   uint32_t* first_range_dev, uint64_t* slots_dev, void* temp_dev, uint64_t temp_bytes,
                                   uint32_t* n_ranges, uint64_t* n_mems, uint64_t* records, void* stream)
{
    NVB_REQUIRE( f_index && r_index && reads && params && n_ranges && n_mems, "NULL argument" );
    *n_ranges = 0; *n_mems = 0;
    if (records) *records = 0;
    DevIndex f, r; int fdev = 0, rdev = 0;
    NVB_CHECK( fm_handle_dev( f_index, &f, &fdev ) );
    NVB_CHECK( fm_handle_dev( r_index, &r, &rdev ) );
    NVB_REQUIRE( fdev == rdev, "the forward and reverse indices live on different devices" );
    NVB_REQUIRE( f.length == r.length && f.L2_0 == r.L2_0 && f.L2_1 == r.L2_1 && f.L2_2 == r.L2_2 && f.L2_3 == r.L2_3 && f.L2_4 == r.L2_4,
                 "the reverse index does not match the forward one (length / L2 differ)" );
    NVB_REQUIRE( params->min_intv >= 1, "min_intv must be >= 1" );
    MemReads q; NVB_CHECK( mem_reads( reads, &q ) );
    DeviceGuard g( fdev ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (q.n == 0)
    {
        if (first_range_dev) NVB_HIP( hipMemsetAsync( first_range_dev, 0, 4, s ) );
        return NVBIO_OK;
    }
    NVB_REQUIRE( first_range_dev && temp_dev, "NULL device pointer" );
    uint64_t total = 0; NVB_CHECK( mem_total( q, s, &total ) );
    // the arena first: its size check covers the whole temp, and its message names what the call needs; the head then ends where it begins
    MemTemp T;
    ScratchBlock arena, head;
    auto take_arena = [&](uint64_t cap) {
        return arena.alloc_layout( "mem_filter_arena", s, "MEM filter: out of device memory", [&](ScratchLayout& c) { T.arena( c, q.n, cap ); },
                                   temp_dev, temp_bytes, "nvbio_mem_filter_temp_bytes", MemTemp::head_end( q.n, total ) );
    };
    NVB_CHECK( take_arena( total ) );
    NVB_CHECK( head.alloc_layout( "mem_filter_head", s, "MEM filter: out of device memory", [&](ScratchLayout& c) { T.head( c, q.n, total ); },
                                  temp_dev, (uint64_t)(arena.get() - (uint8_t*)temp_dev), "nvbio_mem_filter_temp_bytes" ) );

    NVB_HIP( hipMemsetAsync( T.misc, 0, 32, s ) );
    uint64_t* rec = (uint64_t*)(T.misc + 2);
    const uint32_t bits = reads->symbol_bits;
    const bool do_split = params->split_len < 0xFFFFFFFFu;

    // right pass -> candidates per read (mem_reads checked the symbol width: no dispatch below misses)
    NVB_CHECK( with_value( SymbolBits(), bits, [&](auto BITS)
    {
        return NVB_LAUNCH( mem_right_kernel<BITS>, dim3( grid_for( q.n ) ), dim3(256), s, f, r, q, (uint32_t)total, params->min_intv, T.cand, T.cnt,
                           T.misc, rec );
    }, bad_symbol_bits ) );
    NVB_CHECK( scan_u32( T.cnt, T.off, q.n, T, s ) );
    uint32_t n_cand = 0, err = 0;
    NVB_CHECK( read_u32( T.off + q.n, &n_cand, s ) );
    NVB_CHECK( read_u32( T.misc, &err, s ) );
    NVB_REQUIRE( !(err & MEM_ERR_LONG), "a read is longer than 65535 symbols (or the ragged offsets go backwards)" );
    if (err & MEM_ERR_BOUND) { set_error( "MEM filter: internal bound violated in the right pass" ); return NVBIO_ERR_HIP; }

    auto left = [&](uint4* mems, uint32_t n) -> nvbio_status {
        if (n == 0) return NVBIO_OK;
        return with_value( SymbolBits(), bits, [&](auto BITS)
        {
            return NVB_LAUNCH( mem_left_kernel<BITS>, dim3( grid_for( n ) ), dim3(256), s, f, q, mems, n, params->min_intv, rec );
        }, bad_symbol_bits );
    };
    NVB_CHECK( NVB_LAUNCH( mem_gather_kernel, dim3( grid_for( q.n ) ), dim3(256), s, q, (const uint4*)T.cand, T.cnt, T.off, T.dense ) );
    NVB_CHECK( left( T.dense, n_cand ) );
    NVB_CHECK( NVB_LAUNCH( mem_discard_kernel, dim3( grid_for( q.n ) ), dim3(256), s, q.n, (const uint32_t*)T.off, (const uint32_t*)nullptr,
                           T.dense, params->max_intv, params->min_span, T.kept ) );

    const uint4* final_mems = T.dense;
    const uint32_t* final_soff = nullptr;
    if (do_split && n_cand)
    {
        // count (COUNT = true: no arena, no soff), then write into the arena of arena_cap entries
        auto split = [&](auto COUNT, uint4* arena_p, const uint32_t* soff, uint32_t arena_cap) {
            return with_value( SymbolBits(), bits, [&](auto BITS)
            {
                return NVB_LAUNCH( (mem_split_kernel<BITS, COUNT>), dim3( grid_for( n_cand ) ), dim3(256), s, f, r, q, (const uint4*)T.dense, n_cand,
                                   (const uint32_t*)T.off, (const uint32_t*)T.kept, params->split_len, params->split_width, T.scnt, soff, arena_p,
                                   arena_cap, T.misc, rec );
            }, bad_symbol_bits );
        };
        NVB_CHECK( split( std::true_type(), (uint4*)nullptr, (const uint32_t*)nullptr, 0u ) );
        NVB_CHECK( scan_u32( T.scnt, T.soff, n_cand, T, s ) );
        uint32_t n_split = 0;
        NVB_CHECK( read_u32( T.soff + n_cand, &n_split, s ) );
        if (n_split > total) NVB_CHECK( take_arena( n_split ) );     // the split arena is the candidate region: a larger one moves the hipcub temporaries
        NVB_CHECK( split( std::false_type(), T.cand, (const uint32_t*)T.soff, n_split > total ? n_split : (uint32_t)total ) );
        NVB_CHECK( left( T.cand, n_split ) );
        NVB_CHECK( NVB_LAUNCH( mem_discard_kernel, dim3( grid_for( q.n ) ), dim3(256), s, q.n, (const uint32_t*)T.off, (const uint32_t*)T.soff,
                               T.cand, params->max_intv, params->min_span, T.kept ) );
        NVB_CHECK( read_u32( T.misc, &err, s ) );
        if (err & MEM_ERR_BOUND) { set_error( "MEM filter: internal bound violated in the split pass" ); return NVBIO_ERR_HIP; }
        final_mems = T.cand; final_soff = T.soff;
    }

    // output: ranges grouped by string id, first_range = exclusive scan of the kept counts, slots = inclusive scan of the sizes
    NVB_CHECK( scan_u32( T.kept, T.first_tmp, q.n, T, s ) );
    uint32_t nr = 0;
    NVB_CHECK( read_u32( T.first_tmp + q.n, &nr, s ) );
    if (nr > max_ranges)
    {
        set_error( "invalid argument: max_ranges %u too small: this call has %u MEM ranges (ranges_dev and slots_dev need that many entries)",
                   max_ranges, nr );
        *n_ranges = nr;
        return NVBIO_ERR_INVALID;
    }
    NVB_HIP( hipMemcpyAsync( first_range_dev, T.first_tmp, 4ull * (q.n + 1u), hipMemcpyDeviceToDevice, s ) );
    if (nr)
    {
        NVB_REQUIRE( ranges_dev && slots_dev, "NULL device pointer" );
        NVB_CHECK( NVB_LAUNCH( mem_output_kernel, dim3( grid_for( q.n ) ), dim3(256), s, q.n, (const uint32_t*)T.off, final_soff, final_mems,
                               (const uint32_t*)T.first_tmp, (uint4*)ranges_dev ) );
        hipcub::TransformInputIterator<uint64_t, RangeSize, const uint4*> sizes( (const uint4*)ranges_dev, RangeSize() );
        size_t bytes = T.cub_bytes;
        NVB_HIP( hipcub::DeviceScan::InclusiveSum( T.cub, bytes, sizes, slots_dev, (int)nr, s ) );
        NVB_HIP( hipMemcpyAsync( n_mems, slots_dev + (nr - 1u), 8, hipMemcpyDeviceToHost, s ) );
    }
    if (records) NVB_HIP( hipMemcpyAsync( records, rec, 8, hipMemcpyDeviceToHost, s ) );
    NVB_HIP( hipStreamSynchronize( s ) );
    *n_ranges = nr;
    return NVBIO_OK;
}

nvbio_status nvbio_mem_filter_locate(nvbio_fm_index_t f_index, const nvbio_mem_range* ranges_dev, const uint64_t* slots_dev, uint32_t n_ranges,
                                     uint64_t begin, uint64_t end, nvbio_mem_hit* hits_dev, void* stream)
{
    NVB_REQUIRE( f_index != nullptr, "index is NULL" );
    if (end <= begin) return NVBIO_OK;
    NVB_REQUIRE( ranges_dev && slots_dev && hits_dev, "NULL device pointer" );
    NVB_REQUIRE( n_ranges > 0, "locate over an empty filter" );
    DevIndex f; int dev = 0;
    NVB_CHECK( fm_handle_dev( f_index, &f, &dev ) );
    NVB_REQUIRE( f.ssa != nullptr, "index has no sampled suffix array" );
    DeviceGuard g( dev ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    uint64_t n_mems = 0;                                      // an index past the last MEM would read past the ranges
    NVB_HIP( hipMemcpyAsync( &n_mems, slots_dev + (n_ranges - 1u), 8, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
    NVB_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
    NVB_REQUIRE( end <= n_mems, "end is past the last MEM (slots[n_ranges - 1])" );
    return NVB_LAUNCH( mem_locate_kernel, dim3( expand_grid( begin, end ) ), dim3(256),
                       (hipStream_t)stream, f, (const uint4*)ranges_dev, slots_dev, n_ranges, begin, end, (uint4*)hits_dev );
}

} // extern "C"
