// gotoh_banded.hip -- batched banded Gotoh (affine-gap Smith-Waterman) scoring for gfx950.
//
// Reference behaviour reproduced (file:line relative to the reference tree):
//   gotoh_alignment_score_dispatch<BAND,TYPE>::run   nvbio/alignment/gotoh/gotoh_banded_inl.h:397-646
//   row-zero initialisation                          gotoh_banded_inl.h:37-68
//   Reference_cache<BAND> (band-31 2-bit text cache) nvbio/alignment/alignment_base_inl.h:66-90
//   BestSink<int32> (last maximum wins)              nvbio/alignment/sink_inl.h:31-49
//   batched driver (one job per work item)           nvbio/alignment/batched_banded_inl.h:34-157
//   nvBowtie read / window loading                   nvBowtie/bowtie2/cuda/alignment_utils.h:277-302, nvbio/io/utils.h:150-168
//
// MI355X design (integer VALU-bound; MFMA does not apply): one lane owns one alignment and keeps
// the whole band -- H[BAND], F[BAND] -- in VGPRs with every band index a compile-time constant, so
// a row is a straight line of v_add / v_max3 with no LDS traffic, no cross-lane exchange and no
// divergence between lanes of equal read length.  The band-31 text window lives in ONE 64-bit
// register pair (30 x 2 bits) and the per-row match flags for all 30 cached columns come from
// three 64-bit logic ops on it; the LOCAL sink is tracked with one packed (score<<5 | column)
// max per cell and one compare per row, which reproduces BestSink's row-major "last maximum
// wins" rule exactly.  Reads and windows are consumed straight from the packed HBM streams
// (one dword per 8 read symbols / 16 text symbols).
// Band 31 over packed reads in a 2-bit text takes the packed kernel and the end-to-end shortcuts of the band-31 stage instead (band31_jobs.h).
#include "band31_jobs.h"

namespace nvbio_amd {

// BEST2: the cells are reported one by one, in the reference's order, into a Best2Sink<int32>( distinct_dist )
// (sink.h:96-116, sink_inl.h:55-83): best in scores / sinks, the second -- more than distinct_dist text positions away --
// in scores2 / sinks2.  A new best does not demote the old one, so the result depends on the order of the reports.
// STAGED: the result of the staged scheduler (BatchedBandedAlignmentScore<BAND,stream,DeviceStagedThreadScheduler>,
// batched_banded_inl.h:165-236): the windowed banded_alignment_score (gotoh_banded_inl.h:703-727) over 32-row windows
// (batched_stream.h:119,145-180).  The reference re-queues a job after every window to re-compact divergent waves; what that changes
// in the RESULT is (a) the exit at a window's end when no band cell can reach min_score any more (:610-622; LOCAL cells reported so far
// stand, GLOBAL / SEMI_GLOBAL report nothing) and (b) the band passing through int16 checkpoints clamped at int16_min + 32
// (:139-147,166-176).  Here a lane keeps its job for all rows -- lanes that exit idle until the wave ends -- and applies (a) and (b).
template <int BAND, int TYPE, int RBITS, int TBITS, bool BEST2 = false, bool STAGED = false>
__global__ void __launch_bounds__(128)
banded_gotoh_kernel(const BatchDev b, const SchemeDev sc, int32_t* __restrict__ scores, uint2* __restrict__ sinks,
                    const uint32_t distinct_dist, int32_t* __restrict__ scores2, uint2* __restrict__ sinks2,
                    const int32_t* __restrict__ min_scores, const int32_t min_score_all)
{
    __shared__ int32_t s_mm[64];
    fill_mismatch_table( s_mm, sc );

    const uint32_t job = blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= b.n) return;

    // (the header by hand, not load_job + scored_text_len: loading win_end unconditionally costs the LOCAL Best2Sink band-15 build on
    // 8-bit reads two registers, 64 -> 66, and with them a wave; notes/history.md, Round 11)
    const uint32_t rid   = b.read_id ? b.read_id[job] : job;
    const uint32_t first = b.read_offsets[rid];
    const uint32_t M     = b.read_offsets[rid + 1] - first;
    const uint32_t fl    = b.flags ? b.flags[job] : 0u;
    const uint32_t tb    = b.win_begin[job];
    const uint32_t N     = (b.max_read_len && M > b.max_read_len) ? 0u : b.win_end[job] - tb;        // the rule of scored_text_len
    const AlnJob   J{ first, M, tb, N, fl, (fl & NVBIO_READ_REVERSE) != 0, (fl & NVBIO_READ_COMPLEMENT) != 0 };

    int32_t  best   = NVBIO_SCORE_MIN;
    uint32_t best_x = 0xFFFFFFFFu, best_y = 0xFFFFFFFFu;
    int32_t  sec    = NVBIO_SCORE_MIN;                           // BEST2
    uint32_t sec_x  = 0xFFFFFFFFu, sec_y = 0xFFFFFFFFu;
    auto report2 = [&](const int32_t h, const uint32_t x, const uint32_t y) {
        if (best <= h) { best = h; best_x = x; best_y = y; }
        else if (sec <= h && ((uint32_t)(x + distinct_dist) < best_x || x > (uint32_t)(best_x + distinct_dist))) { sec = h; sec_x = x; sec_y = y; }
    };

    if (N < M)                                                   // gotoh_banded_inl.h:422-423: nothing reported
    {
        scores[job] = best; sinks[job] = make_uint2( best_x, best_y );
        if (BEST2) { scores2[job] = sec; sinks2[job] = make_uint2( sec_x, sec_y ); }
        return;
    }

    constexpr bool PACKED = !(BAND == 3 || BAND == 5 || BAND == 7 || BAND == 15);
    static_assert( !PACKED || BAND <= 33, "packed text cache holds at most 32 symbols" );

    SymbolReader<TBITS> trd( b.text );
    SymbolReader<RBITS> prd( b.reads );

    // text cache: columns 0..BAND-2 of the current row
    uint64_t cache_bits = 0;                                     // PACKED: symbol j at bits [2j,2j+1]
    uint32_t cache_raw[PACKED ? 1 : BAND - 1];                   // !PACKED: whole symbols (255 stays 255)
    #pragma unroll
    for (int j = 0; j < BAND - 1; ++j)
    {
        const uint32_t g = ((uint32_t)j < N) ? trd.get( tb + j ) : 255u;
        if (PACKED) cache_bits |= (uint64_t)(g & 3u) << (2 * j);
        else        cache_raw[j] = g;
    }

    const int32_t G_o = sc.pat_go, G_e = sc.pat_ge;             // F: the text advances alone
    const int32_t I_o = sc.ins_go, I_e = sc.ins_ge;             // E: the pattern advances alone (= G for the Gotoh aligner)
    const int32_t infimum = -32768 - max2( max2( G_o, G_e ), max2( sc.txt_go, sc.txt_ge ) );
    const int32_t V = sc.match;

    int32_t H[BAND], F[BAND];
    H[0] = 0;
    #pragma unroll
    for (int j = 1; j < BAND; ++j) H[j] = (TYPE == NVBIO_GLOBAL) ? sc.txt_go + (j - 1) * sc.txt_ge : 0;
    #pragma unroll
    for (int j = 0; j < BAND; ++j) F[j] = infimum;

    bool stopped = false;                                        // STAGED: a window returned false
    const int32_t min_score = STAGED ? (min_scores ? min_scores[job] : min_score_all) : 0;
    for (uint32_t i = 0; i < M; ++i)
    {
        if (STAGED && i && (i & 31u) == 0u)
        {
            int32_t mx = H[0];
            #pragma unroll
            for (int j = 1; j < BAND; ++j) mx = max2( mx, H[j] );
            const int32_t thr = (int32_t)((uint32_t)min_score + (M - i) * (uint32_t)V);
            if (mx < thr) { stopped = true; break; }
            #pragma unroll
            for (int j = 0; j < BAND; ++j)
            {
                H[j] = (int32_t)(int16_t)max2( H[j], -32768 + 32 );
                F[j] = (int32_t)(int16_t)max2( F[j], -32768 + 32 );
            }
        }
        uint32_t pidx;
        const uint32_t q = pattern_symbol( prd, J, i, &pidx );
        const int32_t  S = pattern_mismatch( b.quals, s_mm, pidx );

        // new text symbol entering column BAND-1 (gotoh_banded_inl.h:569-570)
        const uint32_t g_new = (i + (uint32_t)(BAND - 1) < N) ? trd.get( tb + i + (BAND - 1) ) : 255u;

        // per-column match flags of the cached columns
        uint64_t eq_bits = 0;
        if (PACKED)
        {
            if (q < 4u)
            {
                const uint64_t t = cache_bits ^ ((uint64_t)q * 0x5555555555555555ull);
                eq_bits = ~(t | (t >> 1)) & 0x5555555555555555ull;
            }
        }

        int32_t E = 0;
        int32_t row_key = -1;                                    // LOCAL: max over j of (h << 5 | j)
        #pragma unroll
        for (int j = 0; j < BAND; ++j)
        {
            // F from the previous row's column j+1 (:476-479,513-516,575)
            const int32_t f = (j < BAND - 1) ? max2( F[j + 1] + G_e, H[j + 1] + G_o ) : infimum;
            F[j] = f;

            bool eq;
            if (j == BAND - 1)   eq = (g_new == q);
            else if (PACKED)     eq = ((eq_bits >> (2 * j)) & 1ull) != 0;
            else                 eq = (cache_raw[j] == q);
            const int32_t d = H[j] + (eq ? V : S);

            int32_t h;
            if (j == 0)             h = max2( f, d );
            else if (j == BAND - 1) h = max2( E, d );
            else                    h = max3( f, E, d );
            if (TYPE == NVBIO_LOCAL)
            {
                h = max2( h, 0 );
                if (BEST2) report2( h, i + (uint32_t)j + 1u, i + 1u );
                else       row_key = max2( row_key, (h << 5) | j );
            }
            H[j] = h;
            E = (j == 0) ? h + I_o : max2( h + I_o, E + I_e );   // :507,562-565
        }

        // shift the cache by one column and append the new symbol (:532,570)
        if (PACKED) cache_bits = (cache_bits >> 2) | ((uint64_t)(g_new & 3u) << (2 * (BAND - 2)));
        else
        {
            #pragma unroll
            for (int j = 0; j < BAND - 2; ++j) cache_raw[j] = cache_raw[j + 1];
            cache_raw[BAND - 2] = g_new;
        }

        if (TYPE == NVBIO_LOCAL && !BEST2)
        {
            // cells are reported row-major with j ascending and BestSink keeps the LAST maximum
            const int32_t h = row_key >> 5;
            if (h >= best) { best = h; best_x = i + (uint32_t)(row_key & 31) + 1u; best_y = i + 1u; }
        }
    }

    if (STAGED && stopped) { /* nothing more is reported */ }
    else if (TYPE == NVBIO_GLOBAL)                               // :629-630
    {
        if (BEST2) report2( H[BAND - 1], M + BAND - 1, M );
        else if (best <= H[BAND - 1]) { best = H[BAND - 1]; best_x = M + BAND - 1; best_y = M; }
    }
    else if (TYPE == NVBIO_SEMI_GLOBAL)                          // :631-643
    {
        const uint32_t mb = M + (uint32_t)(BAND - 1);
        const uint32_t m  = (mb < N ? mb : N) - (M - 1u);
        #pragma unroll
        for (int j = 0; j < BAND; ++j)
            if (j == 0 || (uint32_t)j < m)
            {
                if (BEST2) report2( H[j], M + j, M );
                else if (best <= H[j]) { best = H[j]; best_x = M + j; best_y = M; }
            }
    }
    scores[job] = best;
    sinks[job]  = make_uint2( best_x, best_y );
    if (BEST2) { scores2[job] = sec; sinks2[job] = make_uint2( sec_x, sec_y ); }
}

template <int BAND>
static nvbio_status launch_score(int type, const BatchDev& b, const SchemeDev& sc, uint32_t rbits, uint32_t tbits,
                                 int32_t* scores, uint2* sinks, hipStream_t s, uint8_t* routes)
{
    return with_value( AlnTypes(), type, [&](auto TYPE)
    {
        if (BAND == 31 && plain_gotoh( sc ) && packed_ok( TYPE, sc, b.max_read_len ) && !(b.algo & NVBIO_ALN_NO_PACKED_DP) &&
            tbits == 2 && (rbits == 4 || rbits == 2))
            return launch_pk( TYPE, rbits, b, sc, scores, sinks, s, routes );
        const dim3 grid( (b.n + 127u) / 128u ), block( 128 );
        return with_bits( BitsAll(), rbits, tbits, [&](auto P)
        {
            return NVB_LAUNCH( (banded_gotoh_kernel<BAND,TYPE,P.r,P.t>), grid, block, s, b, sc, scores, sinks, 0u, nullptr, nullptr, nullptr, 0 );
        }, [&] { return invalid_bits( rbits, tbits ); } );
    }, [&] { return invalid_type( type ); } );
}

template <int BAND>
static nvbio_status launch_staged(int type, const BatchDev& b, const SchemeDev& sc, uint32_t rbits, uint32_t tbits,
                                  const int32_t* min_scores, int32_t min_score, int32_t* scores, uint2* sinks, hipStream_t s)
{
    const dim3 grid( (b.n + 127u) / 128u ), block( 128 );
    return with_value( AlnTypes(), type, [&](auto TYPE)
    {
        return with_bits( BitsStaged(), rbits, tbits, [&](auto P)
        {
            return NVB_LAUNCH( (banded_gotoh_kernel<BAND,TYPE,P.r,P.t,false,true>), grid, block, s, b, sc, scores, sinks,
                               0u, (int32_t*)nullptr, (uint2*)nullptr, min_scores, min_score );
        }, [&] { set_error( "staged scoring: read_bits/text_bits %u/%u not instantiated (4/2, 2/2, 8/8)", rbits, tbits ); return NVBIO_ERR_UNSUPPORTED; } );
    }, [&] { return invalid_type( type ); } );
}

nvbio_status make_batch(const nvbio_alignment_batch* in, BatchDev* b)
{
    NVB_REQUIRE( in != nullptr, "batch is NULL" );
    NVB_REQUIRE( in->read_bits == 2 || in->read_bits == 4 || in->read_bits == 8, "read_bits must be 2, 4 or 8" );
    NVB_REQUIRE( in->text_bits == 2 || in->text_bits == 8, "text_bits must be 2 or 8" );
    NVB_REQUIRE( in->n < (1u << 31), "at most 2^31 - 1 jobs per batch (the job lists are compacted with 32-bit signed counts)" );
    if (in->n)
    {
        NVB_REQUIRE( in->reads_dev && in->read_offsets_dev && in->text_dev && in->win_begin_dev && in->win_end_dev,
                     "NULL device pointer in batch" );
    }
    b->reads = in->reads_dev; b->read_offsets = in->read_offsets_dev; b->quals = in->quals_dev;
    b->read_id = in->read_id_dev; b->flags = in->flags_dev; b->text = in->text_dev;
    b->win_begin = in->win_begin_dev; b->win_end = in->win_end_dev; b->n = in->n; b->max_read_len = in->max_read_len; b->algo = in->algo_flags;
    // the text's bit planes (nvbio_text_planes_build): only with the packed 2-bit text they were built from, and not under the A/B flag
    const bool planes = in->text_planes_dev && in->text_bits == 2 && !(in->algo_flags & NVBIO_ALN_NO_TEXT_PLANES);
    NVB_REQUIRE( !planes || ((uintptr_t)in->text_planes_dev & 127u) == 0, "text_planes_dev must be 128-byte aligned" );
    b->text_planes = planes ? in->text_planes_dev : nullptr;
    return NVBIO_OK;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

template <int BAND>
static nvbio_status launch_best2(int type, const BatchDev& b, const SchemeDev& sc, uint32_t rbits, uint32_t tbits, uint32_t dist,
                                 int32_t* scores, uint2* sinks, int32_t* scores2, uint2* sinks2, hipStream_t s)
{
    const dim3 grid( (b.n + 127u) / 128u ), block( 128 );
    return with_value( AlnTypes(), type, [&](auto TYPE)
    {
        return with_bits( BitsBest2(), rbits, tbits, [&](auto P)
        {
            return NVB_LAUNCH( (banded_gotoh_kernel<BAND,TYPE,P.r,P.t,true>), grid, block, s, b, sc, scores, sinks, dist, scores2, sinks2, nullptr, 0 );
        }, [&] { set_error( "Best2Sink scoring: read_bits/text_bits %u/%u not instantiated (4/2, 2/2, 8/2, 8/8)", rbits, tbits ); return NVBIO_ERR_UNSUPPORTED; } );
    }, [&] { return invalid_type( type ); } );
}

extern "C" nvbio_status nvbio_banded_gotoh_score_best2(int device, uint32_t band, nvbio_alignment_type type,
                                                       const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch, uint32_t distinct_dist,
                                                       int32_t* scores_dev, nvbio_uint2* sinks_dev, int32_t* scores2_dev, nvbio_uint2* sinks2_dev,
                                                       void* stream)
{
    NVB_REQUIRE( scheme != nullptr, "scheme is NULL" );
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    NVB_CHECK( check_band( band, NVBIO_ERR_UNSUPPORTED ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( scores_dev && sinks_dev && scores2_dev && sinks2_dev, "NULL output pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    const SchemeDev sc = scheme_dev( scheme );
    hipStream_t s = (hipStream_t)stream;
    return with_value( Bands(), band, [&](auto BAND)
    {
        return launch_best2<BAND>( type, b, sc, batch->read_bits, batch->text_bits, distinct_dist, scores_dev, (uint2*)sinks_dev, scores2_dev,
                                   (uint2*)sinks2_dev, s );
    }, [] { return NVBIO_ERR_UNSUPPORTED; } );                             // (the band was checked)
}

static nvbio_status banded_score(int device, uint32_t band, int type, const SchemeDev sc, const BatchDev& b, const nvbio_alignment_batch* batch,
                                 int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream, uint8_t* routes_dev = nullptr)
{
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (routes_dev) NVB_HIP( hipMemsetAsync( routes_dev, 1, b.n, s ) );      // (every route but the end-to-end shortcut's: the DP over every job)
    return with_value( Bands(), band, [&](auto BAND)
    {
        return launch_score<BAND>( type, b, sc, batch->read_bits, batch->text_bits, scores_dev, (uint2*)sinks_dev, s, routes_dev );
    }, [] { return NVBIO_ERR_UNSUPPORTED; } );                             // (the band was checked)
}

extern "C" nvbio_status nvbio_banded_gotoh_score_routes(int device, uint32_t band, nvbio_alignment_type type,
                                                        const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                                        int32_t* scores_dev, nvbio_uint2* sinks_dev, uint8_t* routes_dev, void* stream)
{
    NVB_REQUIRE( scheme != nullptr, "scheme is NULL" );
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    NVB_CHECK( check_band( band, NVBIO_ERR_UNSUPPORTED ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( scores_dev && sinks_dev && routes_dev, "NULL output pointer" );
    return banded_score( device, band, type, scheme_dev( scheme ), b, batch, scores_dev, sinks_dev, stream, routes_dev );
}

extern "C" nvbio_status nvbio_banded_gotoh_score(int device, uint32_t band, nvbio_alignment_type type,
                                                 const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                                 int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream)
{
    NVB_REQUIRE( scheme != nullptr, "scheme is NULL" );
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    NVB_CHECK( check_band( band, NVBIO_ERR_UNSUPPORTED ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( scores_dev && sinks_dev, "NULL output pointer" );
    return banded_score( device, band, type, scheme_dev( scheme ), b, batch, scores_dev, sinks_dev, stream );
}

extern "C" nvbio_status nvbio_banded_gap_pairs(int device, const nvbio_alignment_batch* batch, uint32_t* partner_dev, void* stream)
{
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( partner_dev != nullptr, "NULL output pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    return launch_gap_pairs( b, partner_dev, (hipStream_t)stream );
}

extern "C" nvbio_status nvbio_banded_gotoh_score_staged(int device, uint32_t band, nvbio_alignment_type type,
                                                        const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                                        const int32_t* min_scores_dev, int32_t min_score,
                                                        int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream)
{
    NVB_REQUIRE( scheme != nullptr, "scheme is NULL" );
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    NVB_CHECK( check_band( band, NVBIO_ERR_UNSUPPORTED ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( scores_dev && sinks_dev, "NULL output pointer" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const SchemeDev sc = scheme_dev( scheme );
    return with_value( Bands(), band, [&](auto BAND)
    {
        return launch_staged<BAND>( type, b, sc, batch->read_bits, batch->text_bits, min_scores_dev, min_score, scores_dev, (uint2*)sinks_dev, s );
    }, [] { return NVBIO_ERR_UNSUPPORTED; } );                             // (the band was checked)
}

extern "C" nvbio_status nvbio_banded_sw_score(int device, uint32_t band, nvbio_alignment_type type,
                                              const nvbio_sw_scheme* scheme, const nvbio_alignment_batch* batch,
                                              int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream)
{
    NVB_REQUIRE( scheme != nullptr, "scheme is NULL" );
    BatchDev b; NVB_CHECK( make_batch( batch, &b ) );
    NVB_CHECK( check_band( band, NVBIO_ERR_UNSUPPORTED ) );
    if (b.n == 0) return NVBIO_OK;
    NVB_REQUIRE( scores_dev && sinks_dev, "NULL output pointer" );
    // in the band the boundary row runs over the text; with deletion == insertion this is Gotoh(open = extension) and takes
    // the packed kernel and the ungapped shortcut like any other Gotoh scheme
    SchemeDev sc = scheme_dev( scheme, false );
    sc.wide = 0;
    return banded_score( device, band, type, sc, b, batch, scores_dev, sinks_dev, stream );
}
