// The host loops of nvbio_amd/best_approx.hpp (best_approx, best_approx_ragged, best_approx_paired) over DOUBLES of everything they call: the HIP
// runtime over malloc / memcpy and the nvbio_* entry points as functions that only write down how they were called.  The program links neither
// libnvbio_amd.so nor the HIP runtime and needs no GPU; it prints the trace of the calls to stdout:
//   * one line per call: its name and its scalar arguments, structs field by field;
//   * a pointer as [#k size+offset] -- the k-th allocation since the program began, its size, the offset into it --, never as an address (`null`, or
//     `host` for memory the doubles did not hand out);
//   * a host-to-device copy with its byte count and an FNV-1a checksum of the payload.
// The doubles that produce the counters the loops read back follow a fixed rule, so that every loop ends and the several-hits-per-read phase is
// entered: select_multi keeps n_out = 2 n_active / 3 reads with n_out * n_multi hits, read_queue_filter keeps n / 4 reads, select_flagged_indices
// keeps n / 2 hits.
#include <nvbio_amd/best_approx.hpp>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

struct Block { size_t bytes; unsigned id; };
static std::map<const uint8_t*, Block> g_blocks;              // what hipMalloc / hipHostMalloc handed out
static unsigned g_next_id = 0;

static std::string P(const void* p)
{
    if (p == nullptr) return "null";
    auto it = g_blocks.upper_bound( (const uint8_t*)p );
    if (it != g_blocks.begin())
    {
        --it;
        const size_t off = (size_t)((const uint8_t*)p - it->first);
        if (off < it->second.bytes) { std::ostringstream s; s << "[#" << it->second.id << ' ' << it->second.bytes << "+" << off << "]"; return s.str(); }
    }
    return "host";
}
static void put(std::ostringstream&) {}
template <typename A, typename... Rest> static void put(std::ostringstream& s, const A& a, const Rest&... rest) { s << ' ' << a; put( s, rest... ); }
template <typename... Args> static void T(const char* name, const Args&... args)
{
    std::ostringstream s; s << name; put( s, args... );
    puts( s.str().c_str() );
}
static uint32_t fnv1a(const void* p, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 16777619u; }
    return h;
}
static void* block(size_t bytes)
{
    uint8_t* p = (uint8_t*)malloc( bytes ? bytes : 1 );
    memset( p, 0, bytes );
    g_blocks[p] = Block{ bytes, g_next_id++ };
    return p;
}
static void unblock(void* p) { g_blocks.erase( (const uint8_t*)p ); free( p ); }

static std::string S(const nvbio_string_set* q)
{
    std::ostringstream s;
    s << "{sym=" << P( q->symbols_dev ) << " bits=" << q->symbol_bits << " offs=" << P( q->offsets_dev ) << " ranges=" << q->offsets_are_ranges << " fixed_len=" << q->fixed_len
      << " stride=" << q->stride << " n=" << q->n << " seeds_per_string=" << q->seeds_per_string << " seed_interval=" << q->seed_interval
      << " ivals=" << P( q->seed_intervals_dev ) << "}";
    return s.str();
}
static std::string S(const nvbio_seed_hits_params* p)
{
    std::ostringstream s;
    s << "{" << p->seeds_per_read << ' ' << p->first_offset << ' ' << p->seed_interval << ' ' << p->seed_len << ' ' << p->read_len << ' ' << p->max_hits << ' '
      << p->rep_seeds << ' ' << p->max_effort << ' ' << p->min_ext << ' ' << p->max_ext << "}";
    return s.str();
}
static std::string S(const nvbio_ragged_seed_layout* l)
{
    std::ostringstream s;
    s << "{offs=" << P( l->read_offsets_dev ) << " ivals=" << P( l->seed_intervals_dev ) << ' ' << l->seeds_per_read << ' ' << l->seeding_pass << ' ' << l->max_reseed
      << ' ' << l->seed_len << ' ' << l->min_read_len << "}";
    return s.str();
}
static std::string S(const nvbio_hit_queues* h)
{
    std::ostringstream s;
    s << "{idx=" << P( h->idx_queue_dev ) << " read=" << P( h->hit_read_id_dev ) << " seed=" << P( h->hit_seed_dev ) << " loc=" << P( h->hit_loc_dev )
      << " score=" << P( h->hit_score_dev ) << " sink=" << P( h->hit_sink_dev ) << " n=" << h->n << "}";
    return s.str();
}
static std::string S(const nvbio_alignment_batch* b)
{
    std::ostringstream s;
    s << "{reads=" << P( b->reads_dev ) << " bits=" << b->read_bits << " offs=" << P( b->read_offsets_dev ) << " quals=" << P( b->quals_dev ) << " read_id=" << P( b->read_id_dev )
      << " flags=" << P( b->flags_dev ) << " text=" << P( b->text_dev ) << " bits=" << b->text_bits << " wb=" << P( b->win_begin_dev ) << " we=" << P( b->win_end_dev )
      << " n=" << b->n << " max_read_len=" << b->max_read_len << " algo_flags=" << b->algo_flags << "}";
    return s.str();
}
static std::string S(const nvbio_gotoh_scheme* g)
{
    std::ostringstream s;
    s << "{" << g->match << ' ' << g->mm_min << ' ' << g->mm_max << ' ' << g->pat_gap_open << ' ' << g->pat_gap_ext << ' ' << g->txt_gap_open << ' ' << g->txt_gap_ext << "}";
    return s.str();
}
static std::string S(const nvbio_pe_params* p)
{
    std::ostringstream s;
    s << "{" << p->anchor << ' ' << p->anchor_len << ' ' << p->opposite_len << ' ' << p->anchor_perfect_score << ' ' << p->opposite_perfect_score << ' ' << p->anchor_min_score
      << ' ' << p->opposite_min_score << ' ' << p->score_limit << ' ' << p->worst_score << ' ' << p->match << ' ' << p->txt_gap_open << ' ' << p->txt_gap_ext << ' ' << p->band
      << ' ' << p->genome_len << ' ' << p->policy << ' ' << p->min_frag_len << ' ' << p->max_frag_len << ' ' << p->overlap << ' ' << p->unpaired << ' ' << p->max_effort << ' '
      << p->min_ext << ' ' << p->max_ext << "}";
    return s.str();
}
static const char* H(const void* handle) { return handle ? "handle" : "null"; }

extern "C" {

// ---- the HIP runtime over malloc and memcpy ------------------------------------------------------------------------------------------------
hipError_t hipSetDevice(int device) { T( "hipSetDevice", device ); return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) { *p = block( bytes ); T( "hipMalloc", bytes ); return hipSuccess; }
hipError_t hipFree(void* p) { T( "hipFree", P( p ) ); unblock( p ); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) { *p = block( bytes ); T( "hipHostMalloc", bytes, flags ); return hipSuccess; }
hipError_t hipHostFree(void* p) { T( "hipHostFree", P( p ) ); unblock( p ); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    if (kind == hipMemcpyHostToDevice) T( "hipMemcpyAsync", P( dst ), "host", bytes, "H2D", fnv1a( src, bytes ), H( stream ) );
    else                               T( "hipMemcpyAsync", P( dst ), P( src ), bytes, (int)kind, H( stream ) );
    memcpy( dst, src, bytes );
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream)
{
    T( "hipMemsetAsync", P( dst ), value, bytes, H( stream ) );
    memset( dst, value, bytes );
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) { T( "hipStreamSynchronize", H( stream ) ); return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip double"; }

// ---- the library ---------------------------------------------------------------------------------------------------------------------------
const char* nvbio_amd_last_error(void) { return "library double"; }
nvbio_status nvbio_seed_hits_capacity(uint32_t seeds_per_read, uint32_t max_hits, uint32_t* capacity)
{
    *capacity = 2u * seeds_per_read < max_hits ? 2u * seeds_per_read : max_hits;
    T( "nvbio_seed_hits_capacity", seeds_per_read, max_hits, "->", *capacity );
    return NVBIO_OK;
}
nvbio_status nvbio_best_approx_init(int device, uint32_t n_reads, int32_t worst_score, int32_t* best_dev, uint8_t* best_rc_dev, void* stream)
{
    T( "nvbio_best_approx_init", device, n_reads, worst_score, P( best_dev ), P( best_rc_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_best_approx_init_ragged(int device, uint32_t n_reads, const int32_t* min_scores_dev, int32_t* best_dev, uint8_t* best_rc_dev, void* stream)
{
    T( "nvbio_best_approx_init_ragged", device, n_reads, P( min_scores_dev ), P( best_dev ), P( best_rc_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_read_queue_begin(int device, const uint32_t* queue_dev, uint32_t n, uint32_t read_len, uint32_t first_offset, uint32_t top_seed,
                                    uint32_t max_effort_init, uint32_t* seed_offsets_dev, uint32_t* active_dev, uint32_t* trys_dev, void* stream)
{
    T( "nvbio_read_queue_begin", device, P( queue_dev ), n, read_len, first_offset, top_seed, max_effort_init, P( seed_offsets_dev ), P( active_dev ), P( trys_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_read_queue_begin_ragged(int device, const uint32_t* queue_dev, uint32_t n, const nvbio_ragged_seed_layout* layout, uint32_t n_symbols,
                                           uint32_t top_seed, uint32_t max_effort_init, uint32_t* seed_offsets_dev, uint32_t* active_dev, uint32_t* trys_dev,
                                           void* stream)
{
    T( "nvbio_read_queue_begin_ragged", device, P( queue_dev ), n, S( layout ), n_symbols, top_seed, max_effort_init, P( seed_offsets_dev ), P( active_dev ), P( trys_dev ),
       H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_fm_match(nvbio_fm_index_t index, const nvbio_string_set* queries, uint32_t flags, nvbio_uint2* ranges_dev, uint32_t* blocks_dev, void* stream)
{
    T( "nvbio_fm_match", H( index ), S( queries ), flags, P( ranges_dev ), P( blocks_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_seed_hits_map(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, const uint32_t* read_queue_dev,
                                 uint32_t n_reads, const nvbio_seed_hits_params* params, nvbio_uint2* deques_dev, uint32_t* sizes_dev,
                                 uint8_t* reseed_dev, void* stream)
{
    T( "nvbio_seed_hits_map", device, P( fw_ranges_dev ), P( rc_ranges_dev ), P( read_queue_dev ), n_reads, S( params ), P( deques_dev ), P( sizes_dev ), P( reseed_dev ),
       H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_seed_hits_map_ragged(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, const uint32_t* read_queue_dev,
                                        uint32_t n_reads, const nvbio_ragged_seed_layout* layout, uint32_t max_hits, uint32_t rep_seeds,
                                        nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint8_t* reseed_dev, void* stream)
{
    T( "nvbio_seed_hits_map_ragged", device, P( fw_ranges_dev ), P( rc_ranges_dev ), P( read_queue_dev ), n_reads, S( layout ), max_hits, rep_seeds, P( deques_dev ),
       P( sizes_dev ), P( reseed_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_seed_hits_select_multi(int device, const uint32_t* active_in_dev, uint32_t n_active, const uint32_t* trys_dev, uint32_t capacity,
                                          uint32_t n_multi, nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint32_t* active_out_dev,
                                          uint32_t* hits_first_dev, uint32_t* hits_count_dev, const nvbio_hit_queues* hits, uint32_t* counts_dev,
                                          void* stream)
{
    T( "nvbio_seed_hits_select_multi", device, P( active_in_dev ), n_active, P( trys_dev ), capacity, n_multi, P( deques_dev ), P( sizes_dev ), P( active_out_dev ),
       P( hits_first_dev ), P( hits_count_dev ), S( hits ), P( counts_dev ), H( stream ) );
    counts_dev[0] = 2u * n_active / 3u;
    counts_dev[1] = counts_dev[0] * n_multi;
    return NVBIO_OK;
}
nvbio_status nvbio_fm_locate(nvbio_fm_index_t index, const uint32_t* rows_dev, uint32_t n, uint32_t* pos_dev, void* stream)
{
    T( "nvbio_fm_locate", H( index ), P( rows_dev ), n, P( pos_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_seed_hits_loc(int device, const uint32_t* positions_dev, const nvbio_hit_queues* hits, void* stream)
{
    T( "nvbio_seed_hits_loc", device, P( positions_dev ), S( hits ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_score_stream_flatten(int device, const nvbio_hit_queues* hits, const uint32_t* read_index_dev, uint32_t band_len,
                                        uint32_t genome_len, uint32_t reads_reversed, uint32_t* read_id_dev, uint8_t* flags_dev,
                                        uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream)
{
    T( "nvbio_score_stream_flatten", device, S( hits ), P( read_index_dev ), band_len, genome_len, reads_reversed, P( read_id_dev ), P( flags_dev ), P( win_begin_dev ),
       P( win_end_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_banded_gotoh_score(int device, uint32_t band, nvbio_alignment_type type, const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                      int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream)
{
    T( "nvbio_banded_gotoh_score", device, band, (int)type, S( scheme ), S( batch ), P( scores_dev ), P( sinks_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_score_stream_output(int device, const nvbio_hit_queues* hits, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                       const uint32_t* win_begin_dev, int32_t worst_score, void* stream)
{
    T( "nvbio_score_stream_output", device, S( hits ), P( scores_dev ), P( sinks_dev ), P( win_begin_dev ), worst_score, H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_score_reduce_effort_multi(int device, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                             const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, uint32_t read_len, uint32_t n_ext,
                                             const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev, uint32_t* trys_dev,
                                             uint32_t* sizes_dev, void* stream)
{
    T( "nvbio_score_reduce_effort_multi", device, P( active_dev ), n_active, P( hits_first_dev ), P( hits_count_dev ), S( hits ), read_len, n_ext, S( params ), P( best_dev ),
       P( best_rc_dev ), P( trys_dev ), P( sizes_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_score_reduce_effort_multi_ragged(int device, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                                    const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, const uint32_t* read_offsets_dev,
                                                    uint32_t n_ext, const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev,
                                                    uint32_t* trys_dev, uint32_t* sizes_dev, void* stream)
{
    T( "nvbio_score_reduce_effort_multi_ragged", device, P( active_dev ), n_active, P( hits_first_dev ), P( hits_count_dev ), S( hits ), P( read_offsets_dev ), n_ext,
       S( params ), P( best_dev ), P( best_rc_dev ), P( trys_dev ), P( sizes_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_read_queue_filter(int device, const uint32_t* queue_dev, uint32_t n, const uint8_t* read_flags_dev, uint32_t* queue_out_dev,
                                     uint32_t* count_dev, void* stream)
{
    T( "nvbio_read_queue_filter", device, P( queue_dev ), n, P( read_flags_dev ), P( queue_out_dev ), P( count_dev ), H( stream ) );
    count_dev[0] = n / 4u;
    return NVBIO_OK;
}
nvbio_status nvbio_pe_init(int device, uint32_t n_reads, int32_t worst_score_mate1, int32_t worst_score_mate2, int32_t* best_a_dev, int32_t* best_o_dev, void* stream)
{
    T( "nvbio_pe_init", device, n_reads, worst_score_mate1, worst_score_mate2, P( best_a_dev ), P( best_o_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_pe_anchor_flatten(int device, const nvbio_pe_params* params, const nvbio_hit_queues* hits, const int32_t* best_a_dev, const int32_t* best_o_dev,
                                     uint32_t* read_id_dev, uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev,
                                     void* stream)
{
    T( "nvbio_pe_anchor_flatten", device, S( params ), S( hits ), P( best_a_dev ), P( best_o_dev ), P( read_id_dev ), P( flags_dev ), P( win_begin_dev ), P( win_end_dev ),
       P( min_scores_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_pe_anchor_output(int device, const nvbio_pe_params* params, const nvbio_hit_queues* hits, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                    const uint32_t* win_begin_dev, const int32_t* min_scores_dev, int32_t* hit_opposite_score_dev, uint8_t* valid_dev,
                                    void* stream)
{
    T( "nvbio_pe_anchor_output", device, S( params ), S( hits ), P( scores_dev ), P( sinks_dev ), P( win_begin_dev ), P( min_scores_dev ), P( hit_opposite_score_dev ),
       P( valid_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_select_flagged_indices(int device, const uint8_t* flags_dev, uint32_t n, uint32_t* queue_out_dev, uint32_t* count_dev, void* stream)
{
    T( "nvbio_select_flagged_indices", device, P( flags_dev ), n, P( queue_out_dev ), P( count_dev ), H( stream ) );
    count_dev[0] = n / 2u;
    return NVBIO_OK;
}
nvbio_status nvbio_pe_opposite_flatten(int device, const nvbio_pe_params* params, const uint32_t* queue_dev, uint32_t n, const nvbio_hit_queues* hits,
                                       const int32_t* best_a_dev, const int32_t* best_o_dev, uint32_t* read_id_dev, uint8_t* flags_dev,
                                       uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev, void* stream)
{
    T( "nvbio_pe_opposite_flatten", device, S( params ), P( queue_dev ), n, S( hits ), P( best_a_dev ), P( best_o_dev ), P( read_id_dev ), P( flags_dev ), P( win_begin_dev ),
       P( win_end_dev ), P( min_scores_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_full_gotoh_score(int device, nvbio_alignment_type type, int text_blocking, const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_scores_dev, int32_t* scores_dev, nvbio_uint2* sinks_dev,
                                    void* temp_dev, uint64_t temp_bytes, void* stream)
{
    T( "nvbio_full_gotoh_score", device, (int)type, text_blocking, S( scheme ), S( batch ), max_pattern_len, max_text_len, P( min_scores_dev ), P( scores_dev ),
       P( sinks_dev ), P( temp_dev ), temp_bytes, H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_pe_opposite_output(int device, const nvbio_pe_params* params, const uint32_t* queue_dev, uint32_t n, const int32_t* scores_dev,
                                      const nvbio_uint2* sinks_dev, const uint32_t* win_begin_dev, const uint32_t* win_end_dev, const int32_t* min_scores_dev,
                                      int32_t* hit_opposite_score_dev, uint32_t* hit_opposite_loc_dev, uint32_t* hit_opposite_sink_dev, void* stream)
{
    T( "nvbio_pe_opposite_output", device, S( params ), P( queue_dev ), n, P( scores_dev ), P( sinks_dev ), P( win_begin_dev ), P( win_end_dev ), P( min_scores_dev ),
       P( hit_opposite_score_dev ), P( hit_opposite_loc_dev ), P( hit_opposite_sink_dev ), H( stream ) );
    return NVBIO_OK;
}
nvbio_status nvbio_pe_score_reduce(int device, const nvbio_pe_params* params, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                   const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, const int32_t* hit_opposite_score_dev,
                                   const uint32_t* hit_opposite_loc_dev, const uint32_t* hit_opposite_sink_dev, uint32_t n_ext, int32_t* best_a_dev,
                                   int32_t* best_o_dev, uint32_t* trys_dev, uint32_t* sizes_dev, void* stream)
{
    T( "nvbio_pe_score_reduce", device, S( params ), P( active_dev ), n_active, P( hits_first_dev ), P( hits_count_dev ), S( hits ), P( hit_opposite_score_dev ),
       P( hit_opposite_loc_dev ), P( hit_opposite_sink_dev ), n_ext, P( best_a_dev ), P( best_o_dev ), P( trys_dev ), P( sizes_dev ), H( stream ) );
    return NVBIO_OK;
}

} // extern "C"

// the caller's own device arrays: blocks of the doubles, so that the trace names them by size
template <typename U> static U* dev(size_t n) { return (U*)block( n * sizeof(U) ); }

int main()
{
    using namespace nvbio_amd_host;
    const nvbio_fm_index_t fmi = (nvbio_fm_index_t)(uintptr_t)16;         // opaque to the loops
    const hipStream_t stream = (hipStream_t)(uintptr_t)32;
    const nvbio_gotoh_scheme scheme = { 2, 2, 6, -5, -3, -5, -3 };
    const uint32_t R = 64, genome_len = 1000003;
    uint32_t* genome2 = dev<uint32_t>( 4096 );
    BestApproxParams prm;
    prm.max_ext = 30;                                                     // the several-hits-per-read phase runs into the limit of extensions

    {   // uniform 150 bp reads
        puts( "== best_approx: 64 reads of 150 bp" );
        uint32_t* reads = dev<uint32_t>( R * 150 / 8 ); uint8_t* quals = dev<uint8_t>( R * 150 );
        int32_t* best = dev<int32_t>( 4 * R ); uint8_t* best_rc = dev<uint8_t>( R );
        const BestApproxStats s = best_approx( 0, fmi, genome2, genome_len, reads, quals, R, 150, NVBIO_LOCAL, scheme, 40, prm, best, best_rc, stream );
        T( "stats", s.n_extensions, s.passes, s.multi_passes, s.seeding_passes );
        for (void* p : { (void*)reads, (void*)quals, (void*)best, (void*)best_rc }) unblock( p );
    }
    {   // reads of different lengths: one below seed_len, one (25 symbols) with a seed slot in the first two passes only
        puts( "== best_approx_ragged: 64 reads of 15 to 1023 symbols" );
        std::vector<uint32_t> off( R + 1, 0u ); std::vector<int32_t> worst( R );
        uint32_t x = 12345u;
        for (uint32_t r = 0; r < R; ++r)
        {
            x = x * 1664525u + 1013904223u;
            const uint32_t M = r == 5 ? 15u : r == 9 ? 25u : r == 17 ? 1023u : r == 21 ? 22u : 30u + (x >> 16) % 271u;
            off[r + 1] = off[r] + M; worst[r] = -(int32_t)(M / 2u);
        }
        uint32_t* reads = dev<uint32_t>( off[R] / 8 + 1 );
        int32_t* best = dev<int32_t>( 4 * R ); uint8_t* best_rc = dev<uint8_t>( R );
        const BestApproxStats s = best_approx_ragged( 0, fmi, genome2, genome_len, reads, nullptr, R, off.data(), NVBIO_SEMI_GLOBAL, scheme, worst.data(), prm, best, best_rc,
                                                      stream );
        T( "stats", s.n_extensions, s.passes, s.multi_passes, s.seeding_passes );
        puts( "== best_approx_ragged: 3 reads, none long enough to be seeded" );
        const uint32_t off3[4] = { 0, 10, 31, 40 }; const int32_t worst3[3] = { -5, -10, -4 };
        const BestApproxStats s3 = best_approx_ragged( 0, fmi, genome2, genome_len, reads, nullptr, 3, off3, NVBIO_SEMI_GLOBAL, scheme, worst3, prm, best, best_rc, stream );
        T( "stats", s3.n_extensions, s3.passes, s3.multi_passes, s3.seeding_passes );
        puts( "== best_approx_ragged: a read of 1024 symbols is refused" );
        const uint32_t off2[3] = { 0, 100, 1124 };
        try { best_approx_ragged( 0, fmi, genome2, genome_len, reads, nullptr, 2, off2, NVBIO_SEMI_GLOBAL, scheme, worst3, prm, best, best_rc, stream ); puts( "not refused" ); }
        catch (const std::invalid_argument& e) { T( "invalid_argument", e.what() ); }
        for (void* p : { (void*)reads, (void*)best, (void*)best_rc }) unblock( p );
    }
    {   // paired mates of 100 and 150 bp, several hits per read
        puts( "== best_approx_paired: 64 pairs of 100 / 150 bp" );
        const uint32_t lens[2] = { 100, 150 }; const int32_t worst[2] = { 30, 40 };
        const uint32_t* reads[2] = { dev<uint32_t>( R * 100 / 8 ), dev<uint32_t>( R * 150 / 8 ) };
        const uint8_t* quals[2] = { dev<uint8_t>( R * 100 ), nullptr };
        int32_t* best_a = dev<int32_t>( 8 * R ); int32_t* best_o = dev<int32_t>( 8 * R );
        PairedParams pe; pe.max_frag_len = 600;
        BestApproxParams q = prm; q.batch_size = 96; q.top_seed = 1; q.max_effort_init = 20;
        const PairedStats s = best_approx_paired( 0, fmi, genome2, genome_len, reads, quals, R, lens, NVBIO_LOCAL, scheme, worst, q, pe, best_a, best_o, stream );
        T( "stats", s.n_extensions, s.n_opposite, s.passes, s.multi_passes );
        for (const void* p : { (const void*)reads[0], (const void*)reads[1], (const void*)quals[0], (const void*)best_a, (const void*)best_o }) unblock( (void*)p );
    }
    unblock( genome2 );
    if (!g_blocks.empty()) { printf( "LEAK: %zu blocks\n", g_blocks.size() ); return 1; }
    return 0;
}
