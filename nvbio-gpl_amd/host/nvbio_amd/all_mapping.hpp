// all_mapping.hpp -- nvBowtie's all-mapping mode (`--mode all`, bowtie2 -a: every placement of a read within max_dist edits) as a C++ HOST
// loop over the C ABI of libnvbio_amd (include/nvbio_amd.h).
//
// What it replaces: Aligner::all + score_all (nvBowtie/bowtie2/cuda/aligner_all.h:29-139,141-485) for exact seeding (allow_sub = 0) --
// per seed index a map_exact pass, the scan of all SA range sizes, and per batch of hits select_all -> locate -> AllScoreStream -> banded
// DP -> append of the hits that reach min_score -> AllTracebackStream -> finish_alignment.  As the reference's code behaves, its mapper keeps
// the seeds of retry == max_reseed only (mapping_inl.h:627; see csrc/all_mapping.hip), so seed index i sits at stored offset
// max_reseed * (seed_freq / (max_reseed + 1)) + i * seed_freq, for i < read_len / seed_freq while the seed ends inside the read.
//
// Where this differs from the reference, without changing the multiset of alignments:
//   * all seed indices are mapped, scanned and selected in ONE pass (per_seed_passes = 1 walks them one per pass, as the reference does);
//   * accepted hits are appended in hit order -- read-major, ascending read id -- instead of through an atomic ring buffer;
//   * `unique` keeps one hit per (read, strand, locus) of a chunk before the DP (the reference extends a locus once per seed that found
//     it and says so, aligner_all.h:357-358): the result is then the SET of distinct alignments;
//   * the output hook the reference leaves as a TODO (aligner_all.h:478) is the per-chunk callback below.
// finish_alignment_all's re-score under the Smith-Waterman scheme (traceback_inl.h:760-) is left out, as nvbio_finish_alignment leaves
// it out: the score of a record is the banded aligner's.
//
// Order of the result.  unique = 0: hit order (read, seed index, forward before reverse-complement, SA row), so read ids ascend over the
// whole result (within each pass under per_seed_passes).  unique = 1: ascending (read, rc, loc) within a chunk; across chunks read ids
// still ascend, and a record can appear twice only for the one read whose hits straddle a chunk boundary.  Under per_seed_passes a read's
// seeds fall into different passes, so `unique` removes next to nothing there.
//
// The host reads per pass the number of hits, and per chunk the number of accepted hits (and of distinct hits under `unique`), through
// pinned memory; nothing else.  This file holds no device code.
#pragma once
#include <nvbio_amd/best_approx.hpp>
#include <functional>

namespace nvbio_amd_host {

struct AllMappingParams               // nvBowtie's defaults (bowtie2_cuda_driver.cu:86-141)
{
    uint32_t seed_len        = 22;
    uint32_t seed_freq       = 0;     // 0: S(1, 1.15): int( 1 + 1.15 sqrtf( read_len ) )
    uint32_t max_reseed      = 2;     // enters through the seed offset only
    uint32_t max_dist        = 15;    // documentation of min_score = -max_dist; sizes the band when band = 0
    uint32_t band            = 0;     // 0: Aligner::band_length( max_dist ) (aligner.h:149-158)
    nvbio_alignment_type aln_type = NVBIO_SEMI_GLOBAL;      // SEMI_GLOBAL (end-to-end) or LOCAL (score_inl.h:864-885)
    uint32_t hits_per_batch  = 0;     // 0: 2 Mi hits (about 150 bytes of queues per hit, the traceback's direction vectors aside)
    uint32_t unique          = 0;
    uint32_t per_seed_passes = 0;
    uint32_t want_cigars     = 0;
};

struct AllMappingStats { uint64_t n_hits = 0, n_scored = 0, n_alignments = 0; uint32_t chunks = 0; };

// caller arrays in device memory, `capacity` records each; n_alignments may exceed capacity: the records past it are dropped.  With
// want_cigars also win_begin / source / sink / ed / cigars [capacity x cigar_stride] / cigar_lens as nvbio_banded_sw_traceback and
// nvbio_finish_alignment write them, and optionally mds [capacity x mds_stride] / mds_lens.
struct AllMappingOutput
{
    uint64_t     capacity   = 0;
    uint32_t*    read_id    = nullptr;
    uint8_t*     rc         = nullptr;
    uint32_t*    loc        = nullptr;
    int32_t*     score      = nullptr;
    uint32_t*    win_begin  = nullptr;
    nvbio_uint2* source     = nullptr;
    nvbio_uint2* sink       = nullptr;
    uint32_t*    ed         = nullptr;
    uint16_t*    cigars     = nullptr; uint32_t cigar_stride = 0;
    uint32_t*    cigar_lens = nullptr;
    uint8_t*     mds        = nullptr; uint32_t mds_stride = 0;
    uint32_t*    mds_lens   = nullptr;
};

// the accepted records of one chunk, in the loop's own device arrays (valid until the callback returns; the work that fills them is
// enqueued on the loop's stream): records [first, first + n) of the result
struct AllMappingChunk
{
    uint64_t first; uint32_t n;
    const uint32_t* read_id; const uint8_t* rc; const uint32_t* loc; const int32_t* score;
    const uint32_t* win_begin; const nvbio_uint2* source; const nvbio_uint2* sink; const uint32_t* ed;      // NULL without want_cigars
    const uint16_t* cigars; uint32_t cigar_stride; const uint32_t* cigar_lens;
};
typedef std::function<void(const AllMappingChunk&)> AllMappingCallback;

inline uint32_t band_length(const uint32_t max_dist)                 // Aligner::band_length (aligner.h:149-158)
{
    uint32_t band_len = 4;
    while (band_len - 1u < max_dist * 2u + 1u) band_len *= 2u;
    return band_len - 1u;
}

// stored_reads4_dev: the reads as nvBowtie stores them (io::REVERSE), 4-bit packed, read r at symbols [r * read_len, (r+1) * read_len).
// scheme + min_score: the edit-distance scheme (0,-1,-1,-1) with min_score = -max_dist is the mode as the reference ships it
// (aligner_all_ed.cu:37, scoring.h:165,181).  n_reads * read_len must stay below 2^32 (the read index is 32-bit): std::invalid_argument otherwise,
// before anything is launched or written.
inline AllMappingStats all_mapping(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                                   uint32_t n_reads, uint32_t read_len, const nvbio_sw_scheme& scheme, int32_t min_score, const AllMappingParams& prm,
                                   const AllMappingOutput& out, hipStream_t stream, const AllMappingCallback& on_chunk = AllMappingCallback())
{
    using namespace detail;
    AllMappingStats stats;
    const uint32_t R = n_reads, M = read_len;
    const std::vector<uint32_t> ri = uniform_read_index( R, M );
    if (R == 0 || M == 0) return stats;
    hip( hipSetDevice( device ) );
    const uint32_t L = prm.seed_len < M ? prm.seed_len : M;
    const uint32_t S = seed_interval( M, prm.seed_freq );
    const uint32_t first = prm.max_reseed * (S / (prm.max_reseed + 1u));
    const uint32_t max_seeds = M / S;                                                                               // aligner_all.h:72-74
    const uint32_t band = prm.band ? prm.band : band_length( prm.max_dist );
    const uint32_t H = prm.hits_per_batch ? prm.hits_per_batch : (2u << 20);
    const bool cig = prm.want_cigars != 0;
    if (cig && (out.cigar_stride == 0 || (out.capacity && !(out.win_begin && out.source && out.sink && out.ed && out.cigars && out.cigar_lens))))
        throw std::runtime_error( "all_mapping: want_cigars needs win_begin, source, sink, ed, cigars (cigar_stride > 0) and cigar_lens" );
    uint32_t spr_all = 0;                                                                                           // the seed indices that have a seed
    while (spr_all < max_seeds && (uint64_t)first + (uint64_t)spr_all * S + L <= M) ++spr_all;
    if (spr_all == 0) return stats;
    const uint32_t spr_max = prm.per_seed_passes ? 1u : spr_all;

    uint64_t tmp_bytes = 0, b = 0;
    ok( nvbio_all_hits_scan_temp_bytes( R, spr_max, &b ) );  tmp_bytes = b;
    ok( nvbio_all_score_output_temp_bytes( H, &b ) );        if (b > tmp_bytes) tmp_bytes = b;
    if (prm.unique) { ok( nvbio_all_hits_unique_temp_bytes( H, &b ) ); if (b > tmp_bytes) tmp_bytes = b; }
    const uint64_t Hc = cig ? H : 0u, cs = out.cigar_stride, ms = out.mds ? out.mds_stride : 0u;
    DevBuf read_index( 4ull * (R + 1) ), offs( 4ull * R ), fw( 8ull * R * spr_max ), rc( 8ull * R * spr_max ), slots( 16ull * R * spr_max ), tmp( tmp_bytes ),
           h_read( 4ull * H ), h_seed( 4ull * H ), h_loc( 4ull * H ), pos( 4ull * H ), j_read( 4ull * H ), j_flags( H ), j_wb( 4ull * H ), j_we( 4ull * H ),
           j_scores( 4ull * H ), j_sinks( 8ull * H ), c_read( 4ull * H ), c_rc( H ), c_loc( 4ull * H ), c_score( 4ull * H ), t_scores( 4ull * Hc ),
           t_src( 8ull * Hc ), t_sink( 8ull * Hc ), t_ed( 4ull * Hc ), t_cig( 2ull * Hc * cs ), t_lens( 4ull * Hc ), t_mds( Hc * ms ), t_mdslens( 4ull * Hc );
    const Counters<uint64_t> counters( 32 );
    const uint64_t* h_counters = counters.host;
    uint64_t* d_n_hits = counters.dev.as<uint64_t>(); uint64_t* d_count = d_n_hits + 1; uint32_t* d_n_unique = (uint32_t*)(d_n_hits + 2);
    auto fetch = [&]() { counters.fetch( stream, 4 ); };
    hip( hipMemsetAsync( counters.dev.p, 0, 32, stream ) );
    upload( read_index, ri, stream );                                                                               // the read batch's sequence_index

    const uint32_t n_passes = prm.per_seed_passes ? spr_all : 1u;
    for (uint32_t pass = 0; pass < n_passes; ++pass)
    {
        const nvbio_all_hits_params hp = { spr_max, prm.per_seed_passes ? first + pass * S : first, S, L, M };
        // the seeds of this pass, both match_range calls of the exact mapper, the scan of the range sizes
        ok( nvbio_read_queue_begin( device, nullptr, R, M, hp.first_offset, 0u, 0u, offs.as<uint32_t>(), nullptr, nullptr, stream ) );
        nvbio_string_set qs = { stored_reads4_dev, 4u, offs.as<uint32_t>(), 0u, L, M, R * spr_max, spr_max, S, nullptr };
        ok( nvbio_fm_match( fmi, &qs, NVBIO_FM_SCAN_FORWARD, fw.as<nvbio_uint2>(), nullptr, stream ) );
        ok( nvbio_fm_match( fmi, &qs, NVBIO_FM_COMPLEMENT,   rc.as<nvbio_uint2>(), nullptr, stream ) );
        ok( nvbio_all_hits_scan( device, fw.as<nvbio_uint2>(), rc.as<nvbio_uint2>(), R, &hp, slots.as<uint64_t>(), d_n_hits, tmp.p, tmp_bytes, stream ) );
        fetch();
        const uint64_t n_hits = h_counters[0];
        stats.n_hits += n_hits;
        for (uint64_t begin = 0; begin < n_hits; begin += H)
        {
            const uint32_t n = (uint32_t)(n_hits - begin < H ? n_hits - begin : H);
            nvbio_hit_queues hq = { nullptr, h_read.as<uint32_t>(), h_seed.as<uint32_t>(), h_loc.as<uint32_t>(), nullptr, nullptr, n };
            ok( nvbio_all_hits_select( device, fw.as<nvbio_uint2>(), rc.as<nvbio_uint2>(), R, &hp, slots.as<uint64_t>(), begin, begin + n, &hq, stream ) );
            ok( nvbio_fm_locate( fmi, hq.hit_loc_dev, n, pos.as<uint32_t>(), stream ) );
            ok( nvbio_seed_hits_loc( device, pos.as<uint32_t>(), &hq, stream ) );
            if (prm.unique)
            {
                ok( nvbio_all_hits_unique( device, &hq, &hq, d_n_unique, tmp.p, tmp_bytes, stream ) );
                fetch();
                hq.n = (uint32_t)h_counters[2];
            }
            const uint32_t m = hq.n;
            stats.n_scored += m;
            ok( nvbio_score_stream_flatten( device, &hq, read_index.as<uint32_t>(), band, genome_len, 1u, j_read.as<uint32_t>(), j_flags.as<uint8_t>(),
                                            j_wb.as<uint32_t>(), j_we.as<uint32_t>(), stream ) );
            nvbio_alignment_batch batch = { stored_reads4_dev, 4u, read_index.as<uint32_t>(), nullptr, j_read.as<uint32_t>(), j_flags.as<uint8_t>(), genome2_dev, 2u,
                                            j_wb.as<uint32_t>(), j_we.as<uint32_t>(), m, M, 0u };
            ok( nvbio_banded_sw_score( device, band, prm.aln_type, &scheme, &batch, j_scores.as<int32_t>(), j_sinks.as<nvbio_uint2>(), stream ) );
            ok( nvbio_all_score_output( device, &hq, j_scores.as<int32_t>(), min_score, c_read.as<uint32_t>(), c_rc.as<uint8_t>(), c_loc.as<uint32_t>(),
                                        c_score.as<int32_t>(), 0u, H, d_count, tmp.p, tmp_bytes, stream ) );
            fetch();
            const uint32_t acc = (uint32_t)(h_counters[1] - stats.n_alignments);
            if (cig && acc)
            {
                ok( nvbio_all_traceback_flatten( device, c_read.as<uint32_t>(), c_rc.as<uint8_t>(), c_loc.as<uint32_t>(), acc, read_index.as<uint32_t>(), band,
                                                 genome_len, 1u, j_read.as<uint32_t>(), j_flags.as<uint8_t>(), j_wb.as<uint32_t>(), j_we.as<uint32_t>(), stream ) );
                nvbio_alignment_batch tb = batch; tb.n = acc;
                ok( nvbio_banded_sw_traceback( device, band, prm.aln_type, &scheme, &tb, t_scores.as<int32_t>(), t_src.as<nvbio_uint2>(), t_sink.as<nvbio_uint2>(),
                                               t_cig.as<uint16_t>(), out.cigar_stride, t_lens.as<uint32_t>(), 0u, nullptr, 0u, stream ) );
                ok( nvbio_finish_alignment( device, &tb, t_src.as<nvbio_uint2>(), t_cig.as<uint16_t>(), out.cigar_stride, t_lens.as<uint32_t>(), t_ed.as<uint32_t>(),
                                            ms ? t_mds.as<uint8_t>() : nullptr, (uint32_t)ms, ms ? t_mdslens.as<uint32_t>() : nullptr, stream ) );
            }
            // the chunk's records into the caller's arrays, as far as they have room
            const uint64_t at = stats.n_alignments;
            const uint64_t k = at >= out.capacity ? 0u : (out.capacity - at < acc ? out.capacity - at : acc);
            auto put = [&](void* dst, const void* src, uint64_t elem) {
                if (k && dst) hip( hipMemcpyAsync( (uint8_t*)dst + at * elem, src, k * elem, hipMemcpyDeviceToDevice, stream ) );
            };
            put( out.read_id, c_read.p, 4 ); put( out.rc, c_rc.p, 1 ); put( out.loc, c_loc.p, 4 ); put( out.score, c_score.p, 4 );
            if (cig)
            {
                put( out.win_begin, j_wb.p, 4 ); put( out.source, t_src.p, 8 ); put( out.sink, t_sink.p, 8 ); put( out.ed, t_ed.p, 4 );
                put( out.cigars, t_cig.p, 2ull * cs ); put( out.cigar_lens, t_lens.p, 4 );
                if (ms) { put( out.mds, t_mds.p, ms ); put( out.mds_lens, t_mdslens.p, 4 ); }
            }
            if (on_chunk && acc)
            {
                const AllMappingChunk c = { at, acc, c_read.as<uint32_t>(), c_rc.as<uint8_t>(), c_loc.as<uint32_t>(), c_score.as<int32_t>(),
                                            cig ? j_wb.as<uint32_t>() : nullptr, cig ? t_src.as<nvbio_uint2>() : nullptr, cig ? t_sink.as<nvbio_uint2>() : nullptr,
                                            cig ? t_ed.as<uint32_t>() : nullptr, cig ? t_cig.as<uint16_t>() : nullptr, out.cigar_stride,
                                            cig ? t_lens.as<uint32_t>() : nullptr };
                on_chunk( c );
            }
            stats.n_alignments += acc; ++stats.chunks;
        }
    }
    hip( hipStreamSynchronize( stream ) );
    return stats;
}

} // namespace nvbio_amd_host
