// all_mapping.hip -- the data-parallel steps of nvBowtie's all-mapping mode (`--mode all`: every placement of a read within max_dist
// edits), for gfx950:
//         Aligner::all, score_all                                   nvBowtie/bowtie2/cuda/aligner_all.h:29-139,141-485
//         gather_ranges                                             mapping.cu:29-71
//         select_all_kernel                                         select.cu:91-135
//         AllScoreStream::init_context / output                     score_inl.h:591-700
//         AllTracebackStream::init_context                          traceback_inl.h:287-439
// The reference walks one seed index per pass: map_exact with seed_range = (seed, seed + 1) through the multi-retry map_kernel
// (mapping_inl.h:563-634).  As the reference's code behaves, that kernel stores a deque at retry == max_reseed only: its other store
// condition, `range_count == 0 && range_sum < params.rep_seeds * range_count` (:627; && binds before ||), asks for 0 < rep_seeds * 0
// on unsigned values and never holds, and every retry starts from an empty heap (:603).  The one seed of pass `seed` therefore sits
// at stored offset max_reseed * (seed_freq / (max_reseed + 1)) + seed * seed_freq, and a pass whose seed would end past the read
// has none (:611).  A seed with an N is skipped (its match range is empty); the forward hit is pushed before the
// reverse-complemented one, each when its range is not empty (:193-282); one seed per pass never fills a deque of max_hits >= 2.
// The passes share no state, so all seed indices can be taken at once: with the match ranges laid out read-major, then seed index,
// then forward before reverse-complement -- the layout nvbio_seed_hits_map takes -- slot i of the scan belongs to read
// (i / 2) / seeds_per_read, seed (i / 2) % seeds_per_read, strand i & 1, and the two binary searches of select_all (hit -> range ->
// read) become one search and a division.  A range's size is kept in the 20 bits of SeedHit::range_delta (seed_hit.h:217), as
// nvbio_seed_hits_map keeps it: a range of 2^20 rows or more counts size & 0xFFFFF rows, which is what the reference enumerates.
#include "range_expand.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

struct AllHitsView
{
    const uint2* fw;
    const uint2* rc;
    uint32_t     spr, first_off, interval, seed_len, read_len;
};

// the rows slot i contributes: 0 for an empty range (a seed that found nothing or holds an N) and for a seed that ends past the read
struct AllHitsSlotSize
{
    AllHitsView v;
    __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t i) const
    {
        const uint32_t e = i >> 1, j = e % v.spr;
        if ((uint64_t)v.first_off + (uint64_t)j * v.interval + v.seed_len > v.read_len) return 0ull;
        const uint2 g = (i & 1u) ? v.rc[e] : v.fw[e];
        return g.x > g.y ? 0ull : (uint64_t)((g.y + 1u - g.x) & 0xFFFFFu);
    }
};

// ---- select_all_kernel: one lane per hit of [begin, end) ----
__global__ void __launch_bounds__(256)
all_hits_select_kernel(const uint64_t* __restrict__ slots, const uint32_t n_slots, const AllHitsView v, const uint64_t begin, const uint64_t end,
                       uint32_t* __restrict__ hit_read_id, uint32_t* __restrict__ hit_loc, uint32_t* __restrict__ hit_seed)
{
    expand_ranges( slots, n_slots, begin, end, [&](const uint64_t o, const uint32_t i, const uint64_t base)
    {
        if (i >= n_slots) return;                                          // a hit past the scan's total: nothing is written
        const uint32_t e = i >> 1, strand = i & 1u;
        const uint32_t read = e / v.spr, j = e - read * v.spr;
        const uint32_t off = v.first_off + j * v.interval;
        const uint2    g   = strand ? v.rc[e] : v.fw[e];
        const uint32_t pos = strand ? off : v.read_len - off - v.seed_len; // SeedHit::build_flags (mapping_inl.h:241,275)
        const uint64_t k   = o - begin;
        hit_loc[k]     = g.x + (uint32_t)(o - base);                       // hit->front() + hit_id
        hit_read_id[k] = read;
        hit_seed[k]    = (pos & 0x3FFu) | (strand << 13);                  // packed_seed( pos_in_read, index_dir = 0, rc, top_flag = 0 )
    } );
}

// ---- unique: (read_id, rc, loc) as one sortable key, and back ----
__global__ void __launch_bounds__(256)
all_hits_pack_kernel(const uint32_t* __restrict__ hit_read_id, const uint32_t* __restrict__ hit_seed, const uint32_t* __restrict__ hit_loc, const uint32_t n,
                     uint64_t* __restrict__ keys)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        keys[i] = ((uint64_t)hit_read_id[i] << 33) | ((uint64_t)((hit_seed[i] >> 13) & 1u) << 32) | hit_loc[i];
}
__global__ void __launch_bounds__(256)
all_hits_unpack_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ n_keys, const uint32_t n_max, uint32_t* __restrict__ hit_read_id,
                       uint32_t* __restrict__ hit_seed, uint32_t* __restrict__ hit_loc)
{
    const uint32_t n = *n_keys < n_max ? *n_keys : n_max;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const uint64_t k = keys[i];
        hit_read_id[i] = (uint32_t)(k >> 33); hit_seed[i] = ((uint32_t)(k >> 32) & 1u) << 13; hit_loc[i] = (uint32_t)k;
    }
}

// ---- AllScoreStream::output: the hits that reach min_score, appended in work-item order ----
__global__ void __launch_bounds__(256)
all_score_flag_kernel(const int32_t* __restrict__ scores, const uint32_t n, const int32_t min_score, uint8_t* __restrict__ flags)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) flags[i] = scores[i] >= min_score ? 1 : 0;
}
__global__ void __launch_bounds__(256)
all_score_append_kernel(const uint32_t* __restrict__ accepted, const uint32_t* __restrict__ n_accepted, const uint32_t n_max, const uint32_t* __restrict__ idx_queue,
                        const uint32_t* __restrict__ hit_read_id, const uint32_t* __restrict__ hit_seed, const uint32_t* __restrict__ hit_loc,
                        const int32_t* __restrict__ scores, const uint64_t out_offset, const uint64_t out_capacity, uint32_t* __restrict__ out_read_id,
                        uint8_t* __restrict__ out_rc, uint32_t* __restrict__ out_loc, int32_t* __restrict__ out_score, unsigned long long* __restrict__ count)
{
    const uint32_t n = *n_accepted < n_max ? *n_accepted : n_max;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
    {
        const uint64_t slot = out_offset + k;
        if (slot >= out_capacity) break;                                   // dropped; the count is not
        const uint32_t i = accepted[k], idx = idx_queue ? idx_queue[i] : i;
        out_read_id[slot] = hit_read_id[idx]; out_rc[slot] = (uint8_t)((hit_seed[idx] >> 13) & 1u); out_loc[slot] = hit_loc[idx]; out_score[slot] = scores[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count += n;                  // the only access to *count of this launch
}

// ---- AllTracebackStream::init_context: the window of an accepted record, recomputed from its locus ----
__global__ void __launch_bounds__(256)
all_traceback_flatten_kernel(const uint32_t* __restrict__ rec_read_id, const uint8_t* __restrict__ rec_rc, const uint32_t* __restrict__ rec_loc, const uint32_t n,
                             const uint32_t* __restrict__ read_index, const uint32_t band, const uint32_t genome_len, const uint32_t reads_reversed,
                             uint32_t* __restrict__ read_id, uint8_t* __restrict__ flags, uint32_t* __restrict__ wb, uint32_t* __restrict__ we)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const uint32_t rid = rec_read_id[i], rc = rec_rc[i] & 1u, g = rec_loc[i];
        const uint32_t len = read_index[rid + 1u] - read_index[rid];
        const uint32_t b   = g > band / 2u ? g - band / 2u : 0u;
        const uint32_t e   = b + band + len;                               // uint32 arithmetic, as the reference's
        const uint32_t end = e < genome_len ? e : genome_len;
        const bool     bad = b >= genome_len || end < b;                   // the empty-window rule of score_stream_flatten_kernel
        read_id[i] = rid;
        flags[i]   = reads_reversed ? (rc ? (uint8_t)NVBIO_READ_COMPLEMENT : (uint8_t)NVBIO_READ_REVERSE)
                                    : (rc ? (uint8_t)(NVBIO_READ_REVERSE | NVBIO_READ_COMPLEMENT) : (uint8_t)0);
        wb[i] = bad ? 0u : b;
        we[i] = bad ? 0u : end;
    }
}

static nvbio_status all_hits_view(const nvbio_uint2* fw, const nvbio_uint2* rc, uint32_t n_reads, const nvbio_all_hits_params* p, AllHitsView* v, uint32_t* n_slots)
{
    NVB_REQUIRE( p != nullptr, "params is NULL" );
    NVB_REQUIRE( p->seeds_per_read > 0 && p->seed_len > 0, "seeds_per_read and seed_len must be positive" );
    NVB_REQUIRE( p->read_len < 1024u, "SeedHit keeps the seed position in 10 bits (seed_hit.h:217)" );
    NVB_REQUIRE( (uint64_t)p->first_offset + p->seed_len <= p->read_len, "the first seed does not fit the read" );
    NVB_REQUIRE( (uint64_t)p->first_offset + (uint64_t)(p->seeds_per_read - 1u) * p->seed_interval < (1ull << 31), "seed offsets too large" );
    NVB_REQUIRE( 2ull * n_reads * p->seeds_per_read < (1ull << 31), "n_reads x seeds_per_read too large" );
    *v = AllHitsView{ (const uint2*)fw, (const uint2*)rc, p->seeds_per_read, p->first_offset, p->seed_interval, p->seed_len, p->read_len };
    *n_slots = 2u * n_reads * p->seeds_per_read;
    return NVBIO_OK;
}

typedef hipcub::TransformInputIterator<uint64_t, AllHitsSlotSize, hipcub::CountingInputIterator<uint32_t> > SlotSizes;

static nvbio_status all_hits_scan_work_bytes(uint32_t n_slots, size_t* bytes)
{
    const AllHitsView none = { nullptr, nullptr, 1u, 0u, 0u, 1u, 1u };
    SlotSizes sizes( hipcub::CountingInputIterator<uint32_t>( 0u ), AllHitsSlotSize{ none } );
    NVB_HIP( hipcub::DeviceScan::InclusiveSum( nullptr, *bytes, sizes, (uint64_t*)nullptr, (int)n_slots, (hipStream_t)0 ) );
    return NVBIO_OK;
}

// the caller's temp from its first 256-byte boundary on
static inline uint8_t* temp_base(void* temp, uint64_t temp_bytes, uint64_t* left)
{
    const uint64_t skip = (256u - ((uintptr_t)temp & 255u)) & 255u;
    *left = temp_bytes > skip ? temp_bytes - skip : 0u;
    return (uint8_t*)temp + skip;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_all_hits_scan_temp_bytes(uint32_t n_reads, uint32_t seeds_per_read, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    NVB_REQUIRE( 2ull * n_reads * seeds_per_read < (1ull << 31), "n_reads x seeds_per_read too large" );
    size_t work = 0; NVB_CHECK( all_hits_scan_work_bytes( 2u * n_reads * seeds_per_read, &work ) );
    *bytes = ScratchLayout::round( work ) + 256u;
    return NVBIO_OK;
}

nvbio_status nvbio_all_hits_scan(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, uint32_t n_reads,
                                 const nvbio_all_hits_params* params, uint64_t* slots_dev, uint64_t* n_hits_dev, void* temp_dev, uint64_t temp_bytes,
                                 void* stream)
{
    NVB_REQUIRE( n_hits_dev != nullptr, "n_hits_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (n_reads == 0) { NVB_HIP( hipMemsetAsync( n_hits_dev, 0, sizeof(uint64_t), s ) ); return NVBIO_OK; }
    AllHitsView v; uint32_t n_slots = 0; NVB_CHECK( all_hits_view( fw_ranges_dev, rc_ranges_dev, n_reads, params, &v, &n_slots ) );
    NVB_REQUIRE( fw_ranges_dev && rc_ranges_dev && slots_dev, "NULL device pointer" );
    size_t work = 0; NVB_CHECK( all_hits_scan_work_bytes( n_slots, &work ) );
    uint64_t left = 0; uint8_t* base = temp_base( temp_dev, temp_bytes, &left );
    NVB_REQUIRE( temp_dev != nullptr && left >= work, "temp_bytes too small (nvbio_all_hits_scan_temp_bytes)" );
    SlotSizes sizes( hipcub::CountingInputIterator<uint32_t>( 0u ), AllHitsSlotSize{ v } );
    const hipError_t e = hipcub::DeviceScan::InclusiveSum( base, work, sizes, slots_dev, (int)n_slots, s );
    if (e != hipSuccess) { set_error( "all_hits_scan: scan failed: %s", hipGetErrorString( e ) ); return NVBIO_ERR_HIP; }
    NVB_HIP( hipMemcpyAsync( n_hits_dev, slots_dev + (n_slots - 1u), sizeof(uint64_t), hipMemcpyDeviceToDevice, s ) );
    return NVBIO_OK;
}

nvbio_status nvbio_all_hits_select(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, uint32_t n_reads,
                                   const nvbio_all_hits_params* params, const uint64_t* slots_dev, uint64_t begin, uint64_t end,
                                   const nvbio_hit_queues* hits, void* stream)
{
    NVB_REQUIRE( hits != nullptr, "hits is NULL" );
    NVB_REQUIRE( begin <= end, "begin > end" );
    if (begin == end || n_reads == 0) return NVBIO_OK;
    NVB_REQUIRE( end - begin <= hits->n, "the hit queues hold fewer than end - begin hits" );
    AllHitsView v; uint32_t n_slots = 0; NVB_CHECK( all_hits_view( fw_ranges_dev, rc_ranges_dev, n_reads, params, &v, &n_slots ) );
    NVB_REQUIRE( fw_ranges_dev && rc_ranges_dev && slots_dev && hits->hit_read_id_dev && hits->hit_loc_dev && hits->hit_seed_dev, "NULL device pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    return NVB_LAUNCH( all_hits_select_kernel, dim3( expand_grid( begin, end ) ), dim3(256), (hipStream_t)stream, slots_dev, n_slots, v, begin, end,
                       hits->hit_read_id_dev, hits->hit_loc_dev, hits->hit_seed_dev );
}

nvbio_status nvbio_all_hits_unique_temp_bytes(uint32_t n, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    uint64_t su = 0; NVB_CHECK( nvbio_sort_unique_keys_temp_bytes( n, &su ) );
    *bytes = ScratchLayout::round( su ) + ScratchLayout::round( (uint64_t)n * sizeof(uint64_t) ) + 256u;
    return NVBIO_OK;
}

nvbio_status nvbio_all_hits_unique(int device, const nvbio_hit_queues* hits, const nvbio_hit_queues* hits_out, uint32_t* n_out_dev, void* temp_dev,
                                   uint64_t temp_bytes, void* stream)
{
    NVB_REQUIRE( hits != nullptr && hits_out != nullptr && n_out_dev != nullptr, "NULL argument" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = hits->n;
    if (n == 0) { NVB_HIP( hipMemsetAsync( n_out_dev, 0, sizeof(uint32_t), s ) ); return NVBIO_OK; }
    NVB_REQUIRE( hits->idx_queue_dev == nullptr && hits_out->idx_queue_dev == nullptr, "the hit queues must be dense (idx_queue_dev = NULL)" );
    NVB_REQUIRE( hits->hit_read_id_dev && hits->hit_seed_dev && hits->hit_loc_dev && hits_out->hit_read_id_dev && hits_out->hit_seed_dev && hits_out->hit_loc_dev,
                 "NULL device pointer" );
    NVB_REQUIRE( hits_out->n >= n, "the output hit queues hold fewer than hits->n hits" );
    uint64_t su = 0; NVB_CHECK( nvbio_sort_unique_keys_temp_bytes( n, &su ) );
    su = ScratchLayout::round( su );
    uint64_t left = 0; uint8_t* base = temp_base( temp_dev, temp_bytes, &left );
    NVB_REQUIRE( temp_dev != nullptr && left >= su + (uint64_t)n * sizeof(uint64_t), "temp_bytes too small (nvbio_all_hits_unique_temp_bytes)" );
    uint64_t* keys = (uint64_t*)(base + su);                               // the sort's scratch | the keys
    NVB_CHECK( NVB_LAUNCH( all_hits_pack_kernel, dim3( grid_for( n ) ), dim3(256), s, hits->hit_read_id_dev, hits->hit_seed_dev, hits->hit_loc_dev, n, keys ) );
    NVB_CHECK( nvbio_sort_unique_keys( device, keys, n, n_out_dev, base, su, stream ) );
    return NVB_LAUNCH( all_hits_unpack_kernel, dim3( grid_for( n ) ), dim3(256), s, keys, n_out_dev, n, hits_out->hit_read_id_dev, hits_out->hit_seed_dev,
                       hits_out->hit_loc_dev );
}

nvbio_status nvbio_all_score_output_temp_bytes(uint32_t n, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    *bytes = ScratchLayout::round( n ) + ScratchLayout::round( (uint64_t)n * sizeof(uint32_t) ) + 256u + 256u;
    return NVBIO_OK;
}

nvbio_status nvbio_all_score_output(int device, const nvbio_hit_queues* hits, const int32_t* scores_dev, int32_t min_score, uint32_t* out_read_id_dev,
                                    uint8_t* out_rc_dev, uint32_t* out_loc_dev, int32_t* out_score_dev, uint64_t out_offset, uint64_t out_capacity,
                                    uint64_t* count_dev, void* temp_dev, uint64_t temp_bytes, void* stream)
{
    NVB_REQUIRE( hits != nullptr && count_dev != nullptr, "NULL argument" );
    const uint32_t n = hits->n;
    if (n == 0) return NVBIO_OK;
    NVB_REQUIRE( n < (1u << 31), "n too large" );
    NVB_REQUIRE( hits->hit_read_id_dev && hits->hit_seed_dev && hits->hit_loc_dev && scores_dev, "NULL device pointer" );
    NVB_REQUIRE( out_capacity <= out_offset || (out_read_id_dev && out_rc_dev && out_loc_dev && out_score_dev), "NULL output pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    uint64_t left = 0; uint8_t* base = temp_base( temp_dev, temp_bytes, &left );
    const uint64_t at_idx = ScratchLayout::round( n ), at_cnt = at_idx + ScratchLayout::round( (uint64_t)n * sizeof(uint32_t) );
    NVB_REQUIRE( temp_dev != nullptr && left >= at_cnt + 256u, "temp_bytes too small (nvbio_all_score_output_temp_bytes)" );
    uint8_t*  flags    = base;                                             // flags | accepted work items | their number
    uint32_t* accepted = (uint32_t*)(base + at_idx);
    uint32_t* n_acc    = (uint32_t*)(base + at_cnt);
    NVB_CHECK( NVB_LAUNCH( all_score_flag_kernel, dim3( grid_for( n ) ), dim3(256), s, scores_dev, n, min_score, flags ) );
    NVB_CHECK( nvbio_select_flagged_indices( device, flags, n, accepted, n_acc, stream ) );
    return NVB_LAUNCH( all_score_append_kernel, dim3( grid_for( n ) ), dim3(256), s, accepted, n_acc, n, hits->idx_queue_dev, hits->hit_read_id_dev,
                       hits->hit_seed_dev, hits->hit_loc_dev, scores_dev, out_offset, out_capacity, out_read_id_dev, out_rc_dev, out_loc_dev, out_score_dev,
                       (unsigned long long*)count_dev );
}

nvbio_status nvbio_all_traceback_flatten(int device, const uint32_t* rec_read_id_dev, const uint8_t* rec_rc_dev, const uint32_t* rec_loc_dev, uint32_t n,
                                         const uint32_t* read_index_dev, uint32_t band_len, uint32_t genome_len, uint32_t reads_reversed,
                                         uint32_t* read_id_dev, uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream)
{
    if (n == 0) return NVBIO_OK;
    NVB_REQUIRE( rec_read_id_dev && rec_rc_dev && rec_loc_dev && read_index_dev, "NULL device pointer" );
    NVB_REQUIRE( read_id_dev && flags_dev && win_begin_dev && win_end_dev, "NULL output pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    return NVB_LAUNCH( all_traceback_flatten_kernel, dim3( grid_for( n ) ), dim3(256), (hipStream_t)stream, rec_read_id_dev, rec_rc_dev, rec_loc_dev, n,
                       read_index_dev, band_len, genome_len, reads_reversed, read_id_dev, flags_dev, win_begin_dev, win_end_dev );
}

} // extern "C"
