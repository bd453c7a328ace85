// best_approx.hpp -- nvBowtie's best-approx single-end loop as a C++ HOST loop over the C ABI of libnvbio_amd (include/nvbio_amd.h).
//
// What it replaces: Aligner::best_approx + best_approx_score (nvBowtie/bowtie2/cuda/aligner_best_approx.h:39-207,363-667) -- the seeding
// passes with reseeding, and per seeding pass the extension loop select -> locate -> BestScoreStream -> banded DP -> score_reduce, including
// the several-hits-per-read phase the reference switches to once fewer than half a batch of reads are active (:487-510).  Every
// data-parallel step is a kernel behind the C ABI; this file holds no device code.  The host reads two counters per extension pass
// (active reads, selected hits) through pinned memory -- they size the next launches -- and nothing else; queues are allocated once per
// call, at their worst-case size (a batch of reads, BATCH_SIZE hits).
//
// The loop is written ONCE (detail::seed_extend_loop) and has four routes -- best_approx (reads of one length), best_approx_ragged (reads of
// different lengths), best_approx_paired (two mates, the loop once per anchor) and best_approx_paired_ragged (two mates of different lengths) --
// each of which hands it what actually differs: the plan of a seeding pass, how a pass begins and maps its seeds, how the selected hits are
// scored, and the reduce call.
//
// LIMIT of the uniform routes (best_approx, both mates of best_approx_paired, all_mapping): read r starts at symbol r * read_len of the stored
// stream and the read index is 32-bit, so n_reads * read_len must stay below 2^32; a larger batch throws std::invalid_argument before any HIP or
// library call (detail::uniform_read_index).  Split such a batch.
#pragma once
#include <nvbio_amd.h>
#include <hip/hip_runtime_api.h>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace nvbio_amd_host {

struct BestApproxParams              // nvBowtie's defaults (bowtie2_cuda_driver.cu:86-141)
{
    uint32_t seed_len        = 22;
    uint32_t seed_freq       = 0;    // 0: S(1, 1.15): int( 1 + 1.15 sqrtf( read_len ) )
    uint32_t max_hits        = 100;
    uint32_t rep_seeds       = 1000;
    uint32_t max_effort      = 15;
    uint32_t max_effort_init = 15;
    uint32_t min_ext         = 30;
    uint32_t max_ext         = 400;
    uint32_t max_reseed      = 2;
    uint32_t band            = 31;
    uint32_t top_seed        = 0;
    uint32_t batch_size      = 0;    // BATCH_SIZE of the reference's multi-hit rule; 0: the number of reads of the call
    uint32_t multi_hit       = 1;    // 0: always one hit per read and pass
};

struct BestApproxStats { uint64_t n_extensions = 0; uint32_t passes = 0, multi_passes = 0, seeding_passes = 0; };

namespace detail {
inline void ok(nvbio_status st) { if (st != NVBIO_OK) throw std::runtime_error( std::string( "nvbio_amd: " ) + nvbio_amd_last_error() ); }
inline void hip(hipError_t e) { if (e != hipSuccess) throw std::runtime_error( std::string( "hip: " ) + hipGetErrorString( e ) ); }
struct DevBuf
{
    void* p = nullptr;
    explicit DevBuf(size_t bytes, bool wanted = true) { if (wanted) hip( hipMalloc( &p, bytes ? bytes : 16 ) ); }
    ~DevBuf() { if (p) (void)hipFree( p ); }
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    template <typename T> T* as() const { return (T*)p; }
};

// counters the device writes and the host reads back through pinned memory: the round trip that sizes the next launches
template <typename T>
struct Counters
{
    DevBuf dev; T* host = nullptr;
    explicit Counters(size_t bytes) : dev( bytes ) { hip( hipHostMalloc( (void**)&host, bytes, hipHostMallocDefault ) ); }
    ~Counters() { (void)hipHostFree( host ); }
    void fetch(hipStream_t stream, uint32_t words, uint32_t at = 0) const
    {
        hip( hipMemcpyAsync( host + at, dev.as<T>() + at, sizeof(T) * words, hipMemcpyDeviceToHost, stream ) );
        hip( hipStreamSynchronize( stream ) );
    }
};

// SimpleFunc S(1, 1.15) (params.h:87-100) unless seed_freq fixes the interval
inline uint32_t seed_interval(uint32_t read_len, uint32_t seed_freq) { return seed_freq ? seed_freq : (uint32_t)(int32_t)(1.0f + 1.15f * sqrtf( (float)read_len )); }

// the sequence_index of a batch of reads of one length, r * read_len; throws where it does not fit 32 bits, before anything touches the device
inline std::vector<uint32_t> uniform_read_index(uint32_t n_reads, uint32_t read_len)
{
    if ((uint64_t)n_reads * read_len >= (1ull << 32))
        throw std::invalid_argument( "nvbio_amd_host: n_reads * read_len must stay below 2^32 symbols (the read index is 32-bit): split the batch" );
    std::vector<uint32_t> ri( (size_t)n_reads + 1 );
    for (size_t r = 0; r < ri.size(); ++r) ri[r] = (uint32_t)r * read_len;
    return ri;
}
inline void upload(const DevBuf& dst, const std::vector<uint32_t>& words, hipStream_t stream)
{
    hip( hipMemcpyAsync( dst.p, words.data(), 4ull * words.size(), hipMemcpyHostToDevice, stream ) );
    hip( hipStreamSynchronize( stream ) );
}

// what a call of any route fixes once
struct Loop
{
    int device; nvbio_fm_index_t fmi; const uint32_t* genome2_dev; uint32_t genome_len; nvbio_alignment_type aln_type; const nvbio_gotoh_scheme& scheme;
    const BestApproxParams& prm; uint32_t R; hipStream_t stream;
    uint32_t max_effort_init, max_ext, BATCH;
    Loop(int device_, nvbio_fm_index_t fmi_, const uint32_t* genome2_dev_, uint32_t genome_len_, nvbio_alignment_type aln_type_, const nvbio_gotoh_scheme& scheme_,
         const BestApproxParams& prm_, uint32_t R_, hipStream_t stream_)
        : device( device_ ), fmi( fmi_ ), genome2_dev( genome2_dev_ ), genome_len( genome_len_ ), aln_type( aln_type_ ), scheme( scheme_ ), prm( prm_ ), R( R_ ),
          stream( stream_ ), max_effort_init( prm_.max_effort_init > prm_.max_effort ? prm_.max_effort_init : prm_.max_effort ),
          max_ext( prm_.max_ext > prm_.max_effort ? prm_.max_ext : prm_.max_effort ), BATCH( prm_.batch_size ? prm_.batch_size : R_ ) {}
};

// the queues of a call, allocated once at their worst-case size: R reads, H = max( BATCH, R ) hits; the paired route has six more
struct LoopBufs
{
    DevBuf queue_a, queue_b, offs, fw, rc, deques, sizes, reseed, trys, active_a, active_b, hits_first, hits_count, h_read, h_seed, h_loc, h_score, h_sink,
           h_oscore, h_oloc, h_osink, pos, j_read, j_flags, j_wb, j_we, j_min, j_scores, j_sinks, valid, oqueue;
    Counters<uint32_t> counts;
    LoopBufs(const Loop& c, uint64_t n_offs, uint64_t spr_max, uint64_t cap, bool paired) : LoopBufs( c.R, c.BATCH > c.R ? c.BATCH : c.R, n_offs, spr_max, cap, paired ) {}
    LoopBufs(uint64_t R, uint64_t H, uint64_t n_offs, uint64_t spr_max, uint64_t cap, bool paired)
        : queue_a( 4 * R ), queue_b( 4 * R ), offs( 4 * n_offs ), fw( 8 * R * spr_max ), rc( 8 * R * spr_max ), deques( 8 * R * cap ), sizes( 4 * R ), reseed( R ),
          trys( 4 * R ), active_a( 4 * R ), active_b( 4 * R ), hits_first( 4 * R ), hits_count( 4 * R ), h_read( 4 * H ), h_seed( 4 * H ), h_loc( 4 * H ), h_score( 4 * H ),
          h_sink( 4 * H ), h_oscore( 4 * H, paired ), h_oloc( 4 * H, paired ), h_osink( 4 * H, paired ), pos( 4 * H ), j_read( 4 * H ), j_flags( H ), j_wb( 4 * H ),
          j_we( 4 * H ), j_min( 4 * H, paired ), j_scores( 4 * H ), j_sinks( 8 * H ), valid( H, paired ), oqueue( 4 * H, paired ), counts( 16 ) {}
};

// THE LOOP: the seeding passes with reseeding and, per seeding pass, the extension loop select -> locate -> score -> reduce with the
// several-hits-per-read phase.  A route supplies
//   plan( pass )                              -> seeds per read of this seeding pass (0: stop), having set up its own per-pass parameters
//   begin( queue, nq )                        -> the queued reads' seeds as the string set of the two match_range calls (read_queue_begin[_ragged])
//   map( queue, nq )                          the matched ranges into the deques (seed_hits_map[_ragged])
//   score( hq, n_hits )                       everything between seed_hits_loc and the reduce: hit.score / hit.sink of the selected hits
//   reduce( active, n_active, hq, n_ext )     the reduce call
// One host synchronisation per seeding pass (the reseed queue's size) and one per extension pass here (active reads, selected hits).
template <typename Plan, typename Begin, typename Map, typename Score, typename Reduce>
inline BestApproxStats seed_extend_loop(const Loop& c, const LoopBufs& b, Plan plan, Begin begin, Map map, Score score, Reduce reduce)
{
    BestApproxStats stats;
    const BestApproxParams& prm = c.prm;
    const uint32_t* queue = nullptr;              // seed_queues: the reads of this seeding pass (NULL: all of them)
    uint32_t nq = c.R;
    uint32_t* queue_bufs[2] = { b.queue_a.as<uint32_t>(), b.queue_b.as<uint32_t>() };
    for (uint32_t seeding_pass = 0; seeding_pass <= prm.max_reseed && nq; ++seeding_pass)
    {
        const uint32_t spr = plan( seeding_pass );
        if (spr == 0) break;                      // no read has a seed slot in this pass, nor (the first offset grows with the pass) in a later one
        ++stats.seeding_passes;
        uint32_t cap = 0; ok( nvbio_seed_hits_capacity( spr, prm.max_hits, &cap ) );
        // the seeds of the queued reads, both match_range calls of the exact mapper, the deques
        const nvbio_string_set qs = begin( queue, nq );
        ok( nvbio_fm_match( c.fmi, &qs, NVBIO_FM_SCAN_FORWARD, b.fw.as<nvbio_uint2>(), nullptr, c.stream ) );
        ok( nvbio_fm_match( c.fmi, &qs, NVBIO_FM_COMPLEMENT,   b.rc.as<nvbio_uint2>(), nullptr, c.stream ) );
        hip( hipMemsetAsync( b.sizes.p, 0, 4ull * c.R, c.stream ) );
        hip( hipMemsetAsync( b.reseed.p, 0, c.R, c.stream ) );
        map( queue, nq );

        // the extension loop (best_approx_score)
        uint32_t* active_in = b.active_a.as<uint32_t>(); uint32_t* active_out = b.active_b.as<uint32_t>();
        uint32_t n_active = nq, n_ext = 0;
        while (n_active && n_ext < c.max_ext)
        {
            uint32_t n_multi = 1;
            if (prm.multi_hit && n_active <= c.BATCH / 2u)
            {
                const uint32_t left = c.max_ext - n_ext < 4096u ? c.max_ext - n_ext : 4096u;
                n_multi = c.BATCH / n_active < left ? c.BATCH / n_active : left;
                if (n_multi < 1u) n_multi = 1u;
            }
            nvbio_hit_queues hq = { nullptr, b.h_read.as<uint32_t>(), b.h_seed.as<uint32_t>(), b.h_loc.as<uint32_t>(), b.h_score.as<int32_t>(), b.h_sink.as<uint32_t>(), 0u };
            ok( nvbio_seed_hits_select_multi( c.device, active_in, n_active, b.trys.as<uint32_t>(), cap, n_multi, b.deques.as<nvbio_uint2>(), b.sizes.as<uint32_t>(),
                                              active_out, b.hits_first.as<uint32_t>(), b.hits_count.as<uint32_t>(), &hq, b.counts.dev.as<uint32_t>(), c.stream ) );
            b.counts.fetch( c.stream, 2 );
            const uint32_t n_out = b.counts.host[0], n_hits = b.counts.host[1];
            if (n_out == 0) break;
            hq.n = n_hits;
            ok( nvbio_fm_locate( c.fmi, hq.hit_loc_dev, n_hits, b.pos.as<uint32_t>(), c.stream ) );
            ok( nvbio_seed_hits_loc( c.device, b.pos.as<uint32_t>(), &hq, c.stream ) );
            score( hq, n_hits );
            reduce( active_out, n_out, hq, n_ext );
            n_ext += n_multi;
            stats.n_extensions += n_hits; ++stats.passes; if (n_multi > 1u) ++stats.multi_passes;
            std::swap( active_in, active_out );
            n_active = n_out;
        }
        // the reads that asked for reseeding go round again
        uint32_t* next = queue_bufs[seeding_pass & 1u];
        ok( nvbio_read_queue_filter( c.device, queue, nq, b.reseed.as<uint8_t>(), next, b.counts.dev.as<uint32_t>(), c.stream ) );
        b.counts.fetch( c.stream, 1 );
        queue = next; nq = b.counts.host[0];
    }
    return stats;
}

// the seeds of reads of ONE length (best_approx, and either mate of best_approx_paired as the anchor): the plan of a seeding pass, its begin and map
struct UniformSeeds
{
    uint32_t M, L, S, retry_stride;
    nvbio_seed_hits_params sp;
    UniformSeeds(uint32_t read_len, const BestApproxParams& prm)
        : M( read_len ), L( prm.seed_len < M ? prm.seed_len : M ), S( seed_interval( M, prm.seed_freq ) ), retry_stride( S / (prm.max_reseed + 1u) ), sp() {}
    uint32_t spr(uint32_t pass) const { return M >= L + pass * retry_stride ? (M - L - pass * retry_stride) / S + 1u : 0u; }
    uint32_t plan(const Loop& c, uint32_t pass)
    {
        sp = { spr( pass ), pass * retry_stride, S, L, M, c.prm.max_hits, c.prm.rep_seeds, c.prm.max_effort, c.prm.min_ext, c.max_ext };
        return sp.seeds_per_read;
    }
    nvbio_string_set begin(const Loop& c, const LoopBufs& b, const uint32_t* stored_reads4_dev, const uint32_t* queue, uint32_t nq) const
    {
        ok( nvbio_read_queue_begin( c.device, queue, nq, M, sp.first_offset, c.prm.top_seed, c.max_effort_init, b.offs.as<uint32_t>(), b.active_a.as<uint32_t>(),
                                    b.trys.as<uint32_t>(), c.stream ) );
        return { stored_reads4_dev, 4u, b.offs.as<uint32_t>(), 0u, L, M, nq * sp.seeds_per_read, sp.seeds_per_read, S, nullptr };
    }
    void map(const Loop& c, const LoopBufs& b, const uint32_t* queue, uint32_t nq) const
    {
        ok( nvbio_seed_hits_map( c.device, b.fw.as<nvbio_uint2>(), b.rc.as<nvbio_uint2>(), queue, nq, &sp, b.deques.as<nvbio_uint2>(), b.sizes.as<uint32_t>(),
                                 b.reseed.as<uint8_t>(), c.stream ) );
    }
};

// single-end scoring of the selected hits (BestScoreStream): window, banded DP, hit.score / hit.sink
inline void score_single_end(const Loop& c, const LoopBufs& b, const uint32_t* stored_reads4_dev, const uint8_t* quals_dev, const uint32_t* read_index_dev,
                             uint32_t max_read_len, uint32_t algo_flags, const nvbio_hit_queues& hq)
{
    ok( nvbio_score_stream_flatten( c.device, &hq, read_index_dev, c.prm.band, c.genome_len, 1u, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(), b.j_wb.as<uint32_t>(),
                                    b.j_we.as<uint32_t>(), c.stream ) );
    nvbio_alignment_batch batch = { stored_reads4_dev, 4u, read_index_dev, quals_dev, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(), c.genome2_dev, 2u,
                                    b.j_wb.as<uint32_t>(), b.j_we.as<uint32_t>(), hq.n, max_read_len, algo_flags };
    ok( nvbio_banded_gotoh_score( c.device, c.prm.band, c.aln_type, &c.scheme, &batch, b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), c.stream ) );
    ok( nvbio_score_stream_output( c.device, &hq, b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), b.j_wb.as<uint32_t>(), -65536, c.stream ) );
}

// the seeds of a RAGGED batch (best_approx_ragged, and either mate of best_approx_paired_ragged as the anchor).  The constructor takes the host tables
// -- every read's seed interval, per seeding pass the largest seed count of a read, the longest read -- and throws std::invalid_argument for offsets
// that decrease or a read of 1024 symbols or more: before anything touches the device.  read_index_dev / intervals_dev are the caller's uploads.
struct RaggedSeeds
{
    const uint32_t* offsets; uint32_t R, L, min_read_len, Mmax = 0, spr_max = 0; bool has_empty = false;     // has_empty: a read of no symbols
    std::vector<uint32_t> intervals, spr_of;
    const uint32_t* read_index_dev = nullptr; const uint32_t* intervals_dev = nullptr;
    nvbio_ragged_seed_layout lay; nvbio_seed_hits_params sp;
    RaggedSeeds(const std::string& who, uint32_t n_reads, const uint32_t* read_offsets, const BestApproxParams& prm, uint32_t min_read_len_)
        : offsets( read_offsets ), R( n_reads ), L( prm.seed_len ), min_read_len( min_read_len_ ), intervals( n_reads ), spr_of( prm.max_reseed + 1u, 0u ), lay(), sp()
    {
        const uint32_t min_len = min_read_len > L ? min_read_len : L;
        const uint32_t n_pass = prm.max_reseed + 1u;
        // a length is below 1024, so the interval and the seed counts are taken once per LENGTH the batch holds, not once per read
        uint32_t interval_of[1024] = {};                    // 0: the batch holds no read of this length
        for (uint32_t r = 0; r < R; ++r)
        {
            if (read_offsets[r + 1] < read_offsets[r]) throw std::invalid_argument( who + ": read_offsets must not decrease" );
            const uint32_t M = read_offsets[r + 1] - read_offsets[r];
            if (M >= 1024u) throw std::invalid_argument( who + ": a read of 1024 symbols or more (SeedHit keeps the seed position in 10 bits, seed_hit.h:217)" );
            if (interval_of[M] == 0u) { const uint32_t S = seed_interval( M, prm.seed_freq ); interval_of[M] = S ? S : 1u; }
            intervals[r] = interval_of[M];
        }
        has_empty = interval_of[0] != 0u;
        for (uint32_t M = 0; M < 1024u; ++M)
        {
            const uint32_t S = interval_of[M];
            if (S == 0u) continue;
            Mmax = M;
            if (M < min_len) continue;
            for (uint32_t p = 0; p < n_pass; ++p)
            {
                const uint32_t first = p * (S / n_pass);
                if (M < L + first) break;
                const uint32_t spr = (M - L - first) / S + 1u;
                if (spr > spr_of[p]) spr_of[p] = spr;
                if (spr > spr_max) spr_max = spr;
            }
        }
    }
    uint32_t plan(const Loop& c, uint32_t pass)
    {
        const uint32_t spr = spr_of[pass];
        lay = { read_index_dev, intervals_dev, spr, pass, c.prm.max_reseed, L, min_read_len };
        sp = { spr, 0u, 0u, L, Mmax, c.prm.max_hits, c.prm.rep_seeds, c.prm.max_effort, c.prm.min_ext, c.max_ext };
        return spr;
    }
    nvbio_string_set begin(const Loop& c, const LoopBufs& b, const uint32_t* stored_reads4_dev, const uint32_t* queue, uint32_t nq) const
    {
        ok( nvbio_read_queue_begin_ragged( c.device, queue, nq, &lay, offsets[R], c.prm.top_seed, c.max_effort_init, b.offs.as<uint32_t>(), b.active_a.as<uint32_t>(),
                                           b.trys.as<uint32_t>(), c.stream ) );
        return nvbio_string_set{ stored_reads4_dev, 4u, b.offs.as<uint32_t>(), 0u, L, 0u, nq * lay.seeds_per_read, 0u, 0u, nullptr };
    }
    void map(const Loop& c, const LoopBufs& b, const uint32_t* queue, uint32_t nq) const
    {
        ok( nvbio_seed_hits_map_ragged( c.device, b.fw.as<nvbio_uint2>(), b.rc.as<nvbio_uint2>(), queue, nq, &lay, c.prm.max_hits, c.prm.rep_seeds, b.deques.as<nvbio_uint2>(),
                                        b.sizes.as<uint32_t>(), b.reseed.as<uint8_t>(), c.stream ) );
    }
};

// one mate of a paired batch as the DP calls see it
struct MateReads { const uint32_t* stored_reads4_dev; const uint8_t* quals_dev; const uint32_t* read_index_dev; uint32_t max_len; };

// paired scoring of the selected hits (BestAnchorScoreStream, BestOppositeScoreStream): the anchor band-aligned against the pair-derived threshold,
// the opposite mate by full-matrix DP for the hits whose anchor passed (the third counter); -> how many those were.  The two flatten calls are the
// route's: flatten_anchor(), flatten_opposite( n_opp ), over the buffers of `b`.
template <typename FlattenAnchor, typename FlattenOpposite>
inline uint32_t score_paired(const Loop& c, const LoopBufs& b, const nvbio_pe_params& pp, uint32_t max_frag_len, const MateReads& a, const MateReads& o,
                             uint32_t anchor_algo_flags, const nvbio_hit_queues& hq, uint32_t n_hits, FlattenAnchor flatten_anchor, FlattenOpposite flatten_opposite)
{
    flatten_anchor();
    nvbio_alignment_batch ab = { a.stored_reads4_dev, 4u, a.read_index_dev, a.quals_dev, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(), c.genome2_dev,
                                 2u, b.j_wb.as<uint32_t>(), b.j_we.as<uint32_t>(), n_hits, a.max_len, anchor_algo_flags };
    ok( nvbio_banded_gotoh_score( c.device, c.prm.band, c.aln_type, &c.scheme, &ab, b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), c.stream ) );
    ok( nvbio_pe_anchor_output( c.device, &pp, &hq, b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), b.j_wb.as<uint32_t>(), b.j_min.as<int32_t>(),
                                b.h_oscore.as<int32_t>(), b.valid.as<uint8_t>(), c.stream ) );
    ok( nvbio_select_flagged_indices( c.device, b.valid.as<uint8_t>(), n_hits, b.oqueue.as<uint32_t>(), b.counts.dev.as<uint32_t>() + 2, c.stream ) );
    b.counts.fetch( c.stream, 1, 2 );
    const uint32_t n_opp = b.counts.host[2];
    if (n_opp == 0) return 0u;
    flatten_opposite( n_opp );
    nvbio_alignment_batch ob = { o.stored_reads4_dev, 4u, o.read_index_dev, o.quals_dev, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(),
                                 c.genome2_dev, 2u, b.j_wb.as<uint32_t>(), b.j_we.as<uint32_t>(), n_opp, o.max_len, 0u };
    ok( nvbio_full_gotoh_score( c.device, c.aln_type, 0 /* pattern blocking */, &c.scheme, &ob, o.max_len, max_frag_len, b.j_min.as<int32_t>(),
                                b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), nullptr, 0, c.stream ) );
    ok( nvbio_pe_opposite_output( c.device, &pp, b.oqueue.as<uint32_t>(), n_opp, b.j_scores.as<int32_t>(), b.j_sinks.as<nvbio_uint2>(), b.j_wb.as<uint32_t>(),
                                  b.j_we.as<uint32_t>(), b.j_min.as<int32_t>(), b.h_oscore.as<int32_t>(), b.h_oloc.as<uint32_t>(), b.h_osink.as<uint32_t>(), c.stream ) );
    return n_opp;
}
} // namespace detail

// The route for reads of ONE length.
// stored_reads4_dev: the reads as nvBowtie stores them (io::REVERSE), 4-bit packed, read r at symbols [r * read_len, (r+1) * read_len);
// quals_dev: one byte per stored symbol or NULL; best_dev [4 n_reads] int32 (16-byte aligned) / best_rc_dev [n_reads]: see
// nvbio_score_reduce_effort.  worst_score = the scheme's min_score( read_len ) (init_alignments' threshold).
// n_reads * read_len must stay below 2^32: std::invalid_argument otherwise, before anything is launched or written.
inline BestApproxStats best_approx(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                                   const uint8_t* quals_dev, uint32_t n_reads, uint32_t read_len, nvbio_alignment_type aln_type, const nvbio_gotoh_scheme& scheme,
                                   int32_t worst_score, const BestApproxParams& prm, int32_t* best_dev, uint8_t* best_rc_dev, hipStream_t stream)
{
    using namespace detail;
    const uint32_t R = n_reads, M = read_len;
    const std::vector<uint32_t> ri = uniform_read_index( R, M );
    if (R == 0) return BestApproxStats();
    hip( hipSetDevice( device ) );
    const Loop c( device, fmi, genome2_dev, genome_len, aln_type, scheme, prm, R, stream );
    UniformSeeds seeds( M, prm );
    const uint32_t spr_max = seeds.spr( 0 );          // >= 1: seed_len is clamped to the read length
    uint32_t cap = 0; ok( nvbio_seed_hits_capacity( spr_max, prm.max_hits, &cap ) );
    const DevBuf read_index( 4ull * (R + 1) );
    const LoopBufs b( c, R, spr_max, cap, false );
    upload( read_index, ri, stream );
    ok( nvbio_best_approx_init( device, R, worst_score, best_dev, best_rc_dev, stream ) );
    const BestApproxStats stats = seed_extend_loop( c, b,
        [&](uint32_t pass) { return seeds.plan( c, pass ); },
        [&](const uint32_t* queue, uint32_t nq) { return seeds.begin( c, b, stored_reads4_dev, queue, nq ); },
        [&](const uint32_t* queue, uint32_t nq) { seeds.map( c, b, queue, nq ); },
        [&](const nvbio_hit_queues& hq, uint32_t) { score_single_end( c, b, stored_reads4_dev, quals_dev, read_index.as<uint32_t>(), M, 0u, hq ); },
        [&](const uint32_t* active, uint32_t n_active, const nvbio_hit_queues& hq, uint32_t n_ext) {
            ok( nvbio_score_reduce_effort_multi( device, active, n_active, b.hits_first.as<uint32_t>(), b.hits_count.as<uint32_t>(), &hq, M, n_ext, &seeds.sp, best_dev,
                                                 best_rc_dev, b.trys.as<uint32_t>(), b.sizes.as<uint32_t>(), stream ) ); } );
    hip( hipStreamSynchronize( stream ) );
    return stats;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The same loop over reads of DIFFERENT lengths: read r = stored symbols [read_offsets[r], read_offsets[r+1]).  The reference's map_kernel works per
// lane (mapping_inl.h:504-529), so every read gets its own seed interval S_r = seed_freq( M_r ), first offset pass * (S_r / (max_reseed + 1)), seed
// count, forward pos_in_read M_r - off - L, DP window (BestScoreStream reads the read's own range, score_inl.h:102-104), distinct distance M_r / 2
// and worst score min_scores[r].  A read shorter than max( min_read_len, seed_len ) is filtered (:510-514): no seeds, no reseeding, unaligned.
// DIVERGENCE: the reference would seed a read with min_read_len <= M_r < seed_len once with the whole read (:516); here it is filtered.  A read that
// passed the filter but has no seed slot in a pass is flagged for reseeding like any read without hits (:549).  The several-hits-per-read phase is
// unchanged: n_multi is a batch-wide number.  The offsets and thresholds are taken on the HOST -- the loop needs the longest read, every read's seed
// interval and the 10-bit position limit (M_r < 1024, seed_hit.h:217) without a device round trip -- and uploaded once; a batch that breaks the limit
// throws std::invalid_argument before anything is launched or written.  Two pinned counters per extension pass, as in the uniform loop.
// ---------------------------------------------------------------------------------------------------------------------------------------------
inline BestApproxStats best_approx_ragged(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                                          const uint8_t* quals_dev, uint32_t n_reads, const uint32_t* read_offsets, nvbio_alignment_type aln_type,
                                          const nvbio_gotoh_scheme& scheme, const int32_t* min_scores, const BestApproxParams& prm, int32_t* best_dev,
                                          uint8_t* best_rc_dev, hipStream_t stream, uint32_t min_read_len = 12)
{
    using namespace detail;
    const uint32_t R = n_reads;
    if (R == 0) return BestApproxStats();
    if (read_offsets == nullptr || min_scores == nullptr) throw std::invalid_argument( "best_approx_ragged: read_offsets and min_scores are required" );
    if (prm.seed_len == 0) throw std::invalid_argument( "best_approx_ragged: seed_len must be positive" );
    RaggedSeeds seeds( "best_approx_ragged", R, read_offsets, prm, min_read_len );
    hip( hipSetDevice( device ) );
    const Loop c( device, fmi, genome2_dev, genome_len, aln_type, scheme, prm, R, stream );
    const DevBuf read_index( 4ull * (R + 1) ), worst( 4ull * R );
    hip( hipMemcpyAsync( read_index.p, read_offsets, 4ull * (R + 1), hipMemcpyHostToDevice, stream ) );
    hip( hipMemcpyAsync( worst.p, min_scores, 4ull * R, hipMemcpyHostToDevice, stream ) );
    hip( hipStreamSynchronize( stream ) );
    ok( nvbio_best_approx_init_ragged( device, R, worst.as<int32_t>(), best_dev, best_rc_dev, stream ) );
    if (seeds.spr_max == 0) { hip( hipStreamSynchronize( stream ) ); return BestApproxStats(); }

    uint32_t cap = 0; ok( nvbio_seed_hits_capacity( seeds.spr_max, prm.max_hits, &cap ) );
    const DevBuf ivals( 4ull * R );
    const LoopBufs b( c, (uint64_t)R * seeds.spr_max, seeds.spr_max, cap, false );            // one explicit offset per seed
    upload( ivals, seeds.intervals, stream );
    seeds.read_index_dev = read_index.as<uint32_t>(); seeds.intervals_dev = ivals.as<uint32_t>();
    const BestApproxStats stats = seed_extend_loop( c, b,
        [&](uint32_t pass) { return seeds.plan( c, pass ); },
        [&](const uint32_t* queue, uint32_t nq) { return seeds.begin( c, b, stored_reads4_dev, queue, nq ); },
        [&](const uint32_t* queue, uint32_t nq) { seeds.map( c, b, queue, nq ); },
        [&](const nvbio_hit_queues& hq, uint32_t) {
            score_single_end( c, b, stored_reads4_dev, quals_dev, read_index.as<uint32_t>(), seeds.Mmax, NVBIO_ALN_RAGGED_READS, hq ); },
        [&](const uint32_t* active, uint32_t n_active, const nvbio_hit_queues& hq, uint32_t n_ext) {
            ok( nvbio_score_reduce_effort_multi_ragged( device, active, n_active, b.hits_first.as<uint32_t>(), b.hits_count.as<uint32_t>(), &hq, read_index.as<uint32_t>(),
                                                        n_ext, &seeds.sp, best_dev, best_rc_dev, b.trys.as<uint32_t>(), b.sizes.as<uint32_t>(), stream ) ); } );
    hip( hipStreamSynchronize( stream ) );
    return stats;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The PAIRED-END form (Aligner::best_approx, aligner_best_approx_paired.h:84-200 and its best_approx_score, :590-1000): for anchor = mate 1, then
// mate 2: the seeding passes and the extension loop of the single-end form over the ANCHOR mate's seed hits, where a selected hit is scored
// as a pair -- anchor band-aligned against a threshold that tightens with the pairs found so far, the opposite mate by full-matrix DP in its
// fragment window for the hits whose anchor passed, score_reduce_paired keeping the best two pairs (or per-mate bests while unpaired).
// Three counters per extension pass through pinned memory (active reads, selected hits, hits whose anchor passed).
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct PairedParams { uint32_t policy = NVBIO_PE_POLICY_FR, min_frag_len = 0, max_frag_len = 500, overlap = 1, unpaired = 1; };
struct PairedStats  { uint64_t n_extensions = 0, n_opposite = 0; uint32_t passes = 0, multi_passes = 0; };

// stored_reads4_dev[m]: mate m+1 of every pair, stored reversed, 4-bit packed, uniform length read_len[m]; best_a_dev / best_o_dev: [n_reads][2][4] int32
// (see nvbio_pe_params); worst_score[m] = scheme.min_score( read_len[m] ).  n_reads * read_len[m] must stay below 2^32 for both mates: std::invalid_argument
// otherwise, before anything is launched or written.
inline PairedStats best_approx_paired(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* const stored_reads4_dev[2],
                                      const uint8_t* const quals_dev[2], uint32_t n_reads, const uint32_t read_len[2], nvbio_alignment_type aln_type,
                                      const nvbio_gotoh_scheme& scheme, const int32_t worst_score[2], const BestApproxParams& prm, const PairedParams& pe,
                                      int32_t* best_a_dev, int32_t* best_o_dev, hipStream_t stream)
{
    using namespace detail;
    PairedStats stats;
    const uint32_t R = n_reads;
    const std::vector<uint32_t> ri[2] = { uniform_read_index( R, read_len[0] ), uniform_read_index( R, read_len[1] ) };
    if (R == 0) return stats;
    hip( hipSetDevice( device ) );
    const Loop c( device, fmi, genome2_dev, genome_len, aln_type, scheme, prm, R, stream );
    UniformSeeds mate_seeds[2] = { UniformSeeds( read_len[0], prm ), UniformSeeds( read_len[1], prm ) };
    uint32_t spr_max = 1, cap_max = 0;
    for (int m = 0; m < 2; ++m) if (mate_seeds[m].spr( 0 ) > spr_max) spr_max = mate_seeds[m].spr( 0 );
    ok( nvbio_seed_hits_capacity( spr_max, prm.max_hits, &cap_max ) );
    const DevBuf read_index[2] = { DevBuf( 4ull * (R + 1) ), DevBuf( 4ull * (R + 1) ) };
    const LoopBufs b( c, R, spr_max, cap_max, true );                             // one set of queues for both anchors
    for (int m = 0; m < 2; ++m) upload( read_index[m], ri[m], stream );
    ok( nvbio_pe_init( device, R, worst_score[0], worst_score[1], best_a_dev, best_o_dev, stream ) );
    const MateReads mates[2] = { { stored_reads4_dev[0], quals_dev[0], read_index[0].as<uint32_t>(), read_len[0] },
                                 { stored_reads4_dev[1], quals_dev[1], read_index[1].as<uint32_t>(), read_len[1] } };

    for (uint32_t anchor = 0; anchor < 2; ++anchor)
    {
        const uint32_t a = anchor, o = 1u - anchor;
        UniformSeeds& seeds = mate_seeds[a];
        const uint32_t M = read_len[a], Mo = read_len[o];
        const nvbio_pe_params pp = { anchor, M, Mo, scheme.match * (int32_t)M, scheme.match * (int32_t)Mo, worst_score[a], worst_score[o], NVBIO_SCORE_MIN, -65536,
                                     scheme.match, scheme.txt_gap_open, scheme.txt_gap_ext, prm.band, genome_len, pe.policy, pe.min_frag_len, pe.max_frag_len,
                                     pe.overlap, pe.unpaired, prm.max_effort, prm.min_ext, c.max_ext };
        const BestApproxStats s = seed_extend_loop( c, b,
            [&](uint32_t pass) { return seeds.plan( c, pass ); },
            [&](const uint32_t* queue, uint32_t nq) { return seeds.begin( c, b, stored_reads4_dev[a], queue, nq ); },
            [&](const uint32_t* queue, uint32_t nq) { seeds.map( c, b, queue, nq ); },
            [&](const nvbio_hit_queues& hq, uint32_t n_hits) {
                stats.n_opposite += score_paired( c, b, pp, pe.max_frag_len, mates[a], mates[o], 0u, hq, n_hits,
                    [&] { ok( nvbio_pe_anchor_flatten( device, &pp, &hq, best_a_dev, best_o_dev, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(), b.j_wb.as<uint32_t>(),
                                                       b.j_we.as<uint32_t>(), b.j_min.as<int32_t>(), stream ) ); },
                    [&](uint32_t n_opp) { ok( nvbio_pe_opposite_flatten( device, &pp, b.oqueue.as<uint32_t>(), n_opp, &hq, best_a_dev, best_o_dev, b.j_read.as<uint32_t>(),
                                                                         b.j_flags.as<uint8_t>(), b.j_wb.as<uint32_t>(), b.j_we.as<uint32_t>(), b.j_min.as<int32_t>(), stream ) ); } ); },
            [&](const uint32_t* active, uint32_t n_active, const nvbio_hit_queues& hq, uint32_t n_ext) {
                ok( nvbio_pe_score_reduce( device, &pp, active, n_active, b.hits_first.as<uint32_t>(), b.hits_count.as<uint32_t>(), &hq, b.h_oscore.as<int32_t>(),
                                           b.h_oloc.as<uint32_t>(), b.h_osink.as<uint32_t>(), n_ext, best_a_dev, best_o_dev, b.trys.as<uint32_t>(), b.sizes.as<uint32_t>(),
                                           stream ) ); } );
        stats.n_extensions += s.n_extensions; stats.passes += s.passes; stats.multi_passes += s.multi_passes;
    }
    hip( hipStreamSynchronize( stream ) );
    return stats;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The paired loop over mates of DIFFERENT lengths: mate m of pair r = stored symbols [read_offsets[m][r], read_offsets[m][r+1]) of stored_reads4_dev[m].
// The reference is per read throughout (include/nvbio_amd.h, nvbio_pe_ragged), so this is the same algorithm with per-pair tables: per anchor the
// seeds of the single-end ragged route over the ANCHOR mate's offsets (S_r, first_r and the per-pass seed count from the host), the paired route's
// scoring with the ragged flatten calls -- the banded call told the longest anchor mate and NVBIO_ALN_RAGGED_READS, the full-matrix call bounded by the
// longest opposite mate -- and the ragged reduce; nvbio_pe_anchor_output / nvbio_pe_opposite_output read no length and are the uniform route's.  One
// set of queues for both anchors, three pinned counters per extension pass.
// The FILTER is the single-end one and applies to seeding only: a mate with M_r < max( min_read_len, seed_len ) contributes no seeds while it is the
// anchor (an empty deque in every pass, never reseeded) and is still aligned as the opposite mate of its partner's hits; a pair whose both mates are
// filtered ends as initialised.  DIVERGENCE, inherited: the reference would seed a mate with min_read_len <= M_r < seed_len once with the whole read
// (mapping_inl.h:516).  Seeding of an anchor stops only when no read of the batch has a seed slot left.
// REFUSED with std::invalid_argument, before any HIP or library call and with nothing written: missing tables; offsets that decrease; a mate of 1024
// symbols or more in either batch (seed_hit.h:217); an empty mate, M_r == 0 (no placement is defined for it).
// min_scores[m][r] = scheme.min_score( M_r of mate m ); both tables and both offset arrays are HOST arrays.
// ---------------------------------------------------------------------------------------------------------------------------------------------
inline PairedStats best_approx_paired_ragged(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* const stored_reads4_dev[2],
                                             const uint8_t* const quals_dev[2], uint32_t n_reads, const uint32_t* const read_offsets[2], nvbio_alignment_type aln_type,
                                             const nvbio_gotoh_scheme& scheme, const int32_t* const min_scores[2], const BestApproxParams& prm, const PairedParams& pe,
                                             int32_t* best_a_dev, int32_t* best_o_dev, hipStream_t stream, uint32_t min_read_len = 12)
{
    using namespace detail;
    PairedStats stats;
    const uint32_t R = n_reads;
    if (R == 0) return stats;
    if (read_offsets == nullptr || min_scores == nullptr || read_offsets[0] == nullptr || read_offsets[1] == nullptr || min_scores[0] == nullptr || min_scores[1] == nullptr)
        throw std::invalid_argument( "best_approx_paired_ragged: read_offsets and min_scores of both mates are required" );
    if (prm.seed_len == 0) throw std::invalid_argument( "best_approx_paired_ragged: seed_len must be positive" );
    RaggedSeeds mate_seeds[2] = { RaggedSeeds( "best_approx_paired_ragged", R, read_offsets[0], prm, min_read_len ),
                                  RaggedSeeds( "best_approx_paired_ragged", R, read_offsets[1], prm, min_read_len ) };
    if (mate_seeds[0].has_empty || mate_seeds[1].has_empty) throw std::invalid_argument( "best_approx_paired_ragged: an empty mate (no placement is defined for it)" );
    hip( hipSetDevice( device ) );
    const Loop c( device, fmi, genome2_dev, genome_len, aln_type, scheme, prm, R, stream );
    uint32_t spr_max = 1, cap_max = 0;
    for (int m = 0; m < 2; ++m) if (mate_seeds[m].spr_max > spr_max) spr_max = mate_seeds[m].spr_max;
    ok( nvbio_seed_hits_capacity( spr_max, prm.max_hits, &cap_max ) );
    const DevBuf read_index[2] = { DevBuf( 4ull * (R + 1) ), DevBuf( 4ull * (R + 1) ) }, worst[2] = { DevBuf( 4ull * R ), DevBuf( 4ull * R ) },
                 ivals[2] = { DevBuf( 4ull * R ), DevBuf( 4ull * R ) };
    const LoopBufs b( c, (uint64_t)R * spr_max, spr_max, cap_max, true );         // one set of queues for both anchors, one explicit offset per seed
    for (int m = 0; m < 2; ++m)
    {
        hip( hipMemcpyAsync( read_index[m].p, read_offsets[m], 4ull * (R + 1), hipMemcpyHostToDevice, stream ) );
        hip( hipMemcpyAsync( worst[m].p, min_scores[m], 4ull * R, hipMemcpyHostToDevice, stream ) );
        upload( ivals[m], mate_seeds[m].intervals, stream );
        mate_seeds[m].read_index_dev = read_index[m].as<uint32_t>(); mate_seeds[m].intervals_dev = ivals[m].as<uint32_t>();
    }
    const MateReads mates[2] = { { stored_reads4_dev[0], quals_dev[0], read_index[0].as<uint32_t>(), mate_seeds[0].Mmax },
                                 { stored_reads4_dev[1], quals_dev[1], read_index[1].as<uint32_t>(), mate_seeds[1].Mmax } };
    nvbio_pe_ragged rg = { nullptr, nullptr, worst[0].as<int32_t>(), worst[1].as<int32_t>() };
    ok( nvbio_pe_init_ragged( device, R, &rg, best_a_dev, best_o_dev, stream ) );

    for (uint32_t anchor = 0; anchor < 2; ++anchor)
    {
        const uint32_t a = anchor, o = 1u - anchor;
        RaggedSeeds& seeds = mate_seeds[a];
        rg.anchor_offsets_dev = mates[a].read_index_dev; rg.opposite_offsets_dev = mates[o].read_index_dev;
        const nvbio_pe_params pp = { anchor, 0u, 0u, 0, 0, 0, 0, NVBIO_SCORE_MIN, -65536,          // the lengths and scores come from `rg`
                                     scheme.match, scheme.txt_gap_open, scheme.txt_gap_ext, prm.band, genome_len, pe.policy, pe.min_frag_len, pe.max_frag_len,
                                     pe.overlap, pe.unpaired, prm.max_effort, prm.min_ext, c.max_ext };
        const BestApproxStats s = seed_extend_loop( c, b,
            [&](uint32_t pass) { return seeds.plan( c, pass ); },
            [&](const uint32_t* queue, uint32_t nq) { return seeds.begin( c, b, stored_reads4_dev[a], queue, nq ); },
            [&](const uint32_t* queue, uint32_t nq) { seeds.map( c, b, queue, nq ); },
            [&](const nvbio_hit_queues& hq, uint32_t n_hits) {
                stats.n_opposite += score_paired( c, b, pp, pe.max_frag_len, mates[a], mates[o], NVBIO_ALN_RAGGED_READS, hq, n_hits,
                    [&] { ok( nvbio_pe_anchor_flatten_ragged( device, &pp, &rg, &hq, best_a_dev, best_o_dev, b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(),
                                                              b.j_wb.as<uint32_t>(), b.j_we.as<uint32_t>(), b.j_min.as<int32_t>(), stream ) ); },
                    [&](uint32_t n_opp) { ok( nvbio_pe_opposite_flatten_ragged( device, &pp, &rg, b.oqueue.as<uint32_t>(), n_opp, &hq, best_a_dev, best_o_dev,
                                                                                b.j_read.as<uint32_t>(), b.j_flags.as<uint8_t>(), b.j_wb.as<uint32_t>(),
                                                                                b.j_we.as<uint32_t>(), b.j_min.as<int32_t>(), stream ) ); } ); },
            [&](const uint32_t* active, uint32_t n_active, const nvbio_hit_queues& hq, uint32_t n_ext) {
                ok( nvbio_pe_score_reduce_ragged( device, &pp, &rg, active, n_active, b.hits_first.as<uint32_t>(), b.hits_count.as<uint32_t>(), &hq, b.h_oscore.as<int32_t>(),
                                                  b.h_oloc.as<uint32_t>(), b.h_osink.as<uint32_t>(), n_ext, best_a_dev, best_o_dev, b.trys.as<uint32_t>(),
                                                  b.sizes.as<uint32_t>(), stream ) ); } );
        stats.n_extensions += s.n_extensions; stats.passes += s.passes; stats.multi_passes += s.multi_passes;
    }
    hip( hipStreamSynchronize( stream ) );
    return stats;
}

} // namespace nvbio_amd_host
