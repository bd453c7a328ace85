// band31_stage.hip -- the host side of the band-31 scoring stage for gfx950: which passes run for a scheme and a batch, in which order and over
// which job lists (launch_pk), the length sort of the DP's list for ragged batches and the route report.  The passes' kernels live in their own
// units (band31_jobs.h declares their launchers); this is the only unit of the stage that takes hipcub in.
#include "band31_jobs.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

// host-side conditions of the shortcut: SEMI_GLOBAL, match = 0, one mismatch penalty for every quality,
// non-positive gap terms
static bool ungapped_ok(const SchemeDev& sc, const BatchDev& b, int32_t* P, bool* by_quality)
{
    if (sc.match != 0) return false;
    if (sc.mm_min < 0 || sc.mm_max < 0) return false;
    // a mismatch that costs nothing (mm_min = 0; a batch without qualities is charged mm_min whatever mm_max is): every diagonal scores 0, and
    // BestSink's last maximum is the last reportable column, not the diagonal with the fewest mismatches the first pass would report
    if (sc.mm_min == 0) return false;
    // the penalty depends on the row (nvBowtie's default: 2..6 by base quality): the first pass sums the candidates' rows exactly
    // (QUAL); it needs a ramp that does not decrease with the quality and a smallest penalty > 0
    *by_quality = b.quals != nullptr && sc.mm_min != sc.mm_max;
    if (*by_quality && (sc.mm_min <= 0 || sc.mm_max < sc.mm_min || (b.algo & NVBIO_ALN_NO_QUALITY_SHORTCUT))) return false;
    if (sc.pat_go >= 0 || sc.txt_go >= 0 || sc.pat_ge > 0 || sc.txt_ge > 0) return false;
    *P = sc.mm_min;                                               // quality 0 / constant ramp: mismatch = -mm_min
    return true;
}

// the narrow classes' thresholds for a scheme (band31_jobs.h: NarrowRule); on = false: the route is off
static NarrowRule narrow_rule(const bool on, const int32_t P, const int32_t go, const int32_t ge)
{
    NarrowRule r = { 1, 1, 0u };
    if (!on || ge >= 0 || P <= 0) return r;
    const int64_t a = (int64_t)go + (int64_t)NARROW_A_HALF * ge + 1, bb = (int64_t)go + (int64_t)NARROW_B_HALF * ge + 1;
    if (bb < -2000) return r;                                      // (far outside what the binary16 lanes are admitted for)
    r.thr_a = (int32_t)a; r.thr_b = (int32_t)bb;
    r.cnt_max = (uint32_t)((-bb) / P);
    return r;
}
static GapLadder gap_ladder(const int32_t P, const int32_t G, const int32_t go, const int32_t ge)
{
    const int64_t floor_u = 3 * (int64_t)(G < go ? G : go) - P;
    const int32_t cap = P > 0 ? (int32_t)((-floor_u - 1) / (int64_t)P) : 0;      // (P <= 0: the first pass sends no job to the gap chance)
    GapLadder l;
    l.c_unk_u = gap_chance_unknown_cost( P, go, ge );
    l.c_unk_n = (cap + 1) * P < l.c_unk_u ? (cap + 1) * P : l.c_unk_u;
    return l;
}

// RAGGED batches: the DP's job list in ascending order of read length, so that the two alignments of a lane -- and the lanes of a wave --
// (nearly always) run the same number of rows: sort key = the job's read length, 0xFFFF behind the list's end (jobs = NULL: every job of
// the batch).  One or two radix passes over (uint16 key, uint32 job).
__global__ void __launch_bounds__(256)
job_length_keys_kernel(const BatchDev b, const uint32_t* __restrict__ jobs, const uint32_t* __restrict__ job_count, uint16_t* __restrict__ keys,
                       uint32_t* __restrict__ jobs_all, uint32_t* __restrict__ count_all)
{
    const uint32_t n = jobs ? *job_count : b.n;
    if (!jobs && blockIdx.x == 0 && threadIdx.x == 0) *count_all = b.n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n; i += gridDim.x * blockDim.x)
    {
        uint32_t key = 0xFFFFu;
        if (i < n)
        {
            const uint32_t job = jobs ? jobs[i] : i;
            const uint32_t M = read_len( b, job );
            key = M < 0xFFFEu ? M : 0xFFFEu;
        }
        keys[i] = (uint16_t)key;
        if (!jobs) jobs_all[i] = i;
    }
}

// sorted list and its length (device) in *list_out / *count_out, both in *aux: the caller keeps it until the work that reads them is enqueued
static nvbio_status sort_jobs_by_length(const BatchDev& b, const uint32_t* job_list, const uint32_t* job_count, const uint32_t** list_out,
                                        const uint32_t** count_out, ScratchBlock* aux, hipStream_t s)
{
    size_t sort_bytes = 0;
    const int bits = 16;                         // (the 0xFFFF keys behind the list's end must sort last: all 16 bits)
    NVB_HIP( hipcub::DeviceRadixSort::SortPairs( nullptr, sort_bytes, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (int)b.n, 0, bits, s ) );
    uint16_t *k_in, *k_out; uint32_t *l_all, *l_out, *c_all; void* tmp;
    NVB_CHECK( aux->alloc_layout( "banded_length_sort", s, "banded score: out of device memory for the length-sorted job list", [&](ScratchLayout& c)
    {
        k_in  = c.take<uint16_t>( b.n ); k_out = c.take<uint16_t>( b.n );
        l_all = c.take<uint32_t>( b.n ); l_out = c.take<uint32_t>( b.n );
        c_all = c.take<uint32_t>( 1 );
        tmp   = c.take<uint8_t>( sort_bytes );
    } ) );
    NVB_CHECK( NVB_LAUNCH( job_length_keys_kernel, dim3( (b.n + 255u) / 256u < 65536u ? (b.n + 255u) / 256u : 65536u ), dim3( 256 ), s, b, job_list, job_count, k_in, l_all, c_all ) );
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs( tmp, sort_bytes, (const uint16_t*)k_in, k_out, job_list ? job_list : (const uint32_t*)l_all, l_out, (int)b.n, 0, bits, s );
    if (e != hipSuccess) { set_error( "job sort failed: %s", hipGetErrorString( e ) ); return NVBIO_ERR_HIP; }
    *list_out = l_out; *count_out = job_list ? job_count : c_all;
    return NVBIO_OK;
}

// the route report's bytes (nvbio_banded_gotoh_score_routes; zeroed before): 1 for the jobs of the DP's full list, 3 / 2 for class B / A;
// REDO: +8 for the jobs of the redo list
template <bool REDO>
__global__ void __launch_bounds__(256)
job_routes_kernel(const JobLists l, const uint32_t n, const bool classes, uint8_t* __restrict__ routes)
{
    const uint32_t n_dp = REDO ? 0u : *l.count( JOB_DP ), n_b = (REDO || !classes) ? 0u : *l.count( JOB_CLASS_B ), n_a = (REDO || !classes) ? 0u : *l.count( JOB_CLASS_A );
    const uint32_t n_r = (REDO && classes) ? *l.count( JOB_REDO ) : 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        if (i < n_dp) routes[l.dp[i]] = 1u;
        if (i < n_b)  routes[l.class_b[i]] = 3u;
        if (i < n_a)  routes[l.class_a[i]] = 2u;
        if (i < n_r)  routes[l.redo[i]] |= 8u;
    }
}

nvbio_status launch_pk(const int type, const uint32_t rbits, const BatchDev& b, const SchemeDev& sc, int32_t* scores, uint2* sinks, hipStream_t s, uint8_t* routes)
{
    const uint32_t pairs = (b.n + 1u) / 2u;
    int32_t P = 0; bool by_quality = false;
    const bool sorted_lengths = type == NVBIO_SEMI_GLOBAL && sc.match == 0 && (b.algo & NVBIO_ALN_RAGGED_READS) && !(b.algo & NVBIO_ALN_NO_LENGTH_SORT);
    // (txt_go / txt_ge never enter the banded recurrences -- both gap recurrences take the pattern-gap terms, gotoh_common.h:23-30 -- which is
    // why the chance kernels below are handed pat_go / pat_ge only; plain_gotoh() at the call site guarantees it.  A scheme that separates
    // the two must disable the shortcut, as gotoh_full.hip does with `second_chance`.)
    if (type == NVBIO_SEMI_GLOBAL && ungapped_ok( sc, b, &P, &by_quality ) && !(b.algo & NVBIO_ALN_NO_UNGAPPED_SCORE))
    {
        // 1. settle the jobs whose best diagonal beats every gapped alignment, 2. give the ones a chance can still settle to that chance,
        // 3. DP over the rest.  Every kernel puts the jobs it does not settle on the list of the launch that takes them next (JobAppend).
        const int32_t G = sc.pat_go > sc.txt_go ? sc.pat_go : sc.txt_go;
        const bool third = !(b.algo & NVBIO_ALN_NO_THIRD_CHANCE);
        uint8_t* need_dp; JobLists out;
        // the DP's narrow classes: formed only where the DP that follows is the binary16 build over a batch without qualities that is not declared ragged
        const NarrowRule nr = narrow_rule( b.quals == nullptr && !(b.algo & (NVBIO_ALN_NO_NARROW_DP | NVBIO_ALN_RAGGED_READS)) && pk_binary16_ok( type, b, sc ),
                                           P, sc.pat_go, sc.pat_ge );
        const bool classes = nr.thr_b != 1;
        ScratchBlock aux;
        NVB_CHECK( aux.alloc_layout( "banded_job_list", s, "banded score: out of device memory for the job list", [&](ScratchLayout& c)
        {
            need_dp     = c.take<uint8_t>( b.n );
            out.dp      = c.take<uint32_t>( b.n );                                           // the DP's jobs
            out.second  = c.take<uint32_t>( b.n );                                           // second-chance jobs
            out.third   = c.take<uint32_t>( b.n );                                           // third-chance / gap-chance jobs
            out.pairs   = c.take<uint32_t>( (b.n + 1u) / 2u );                               // the gap chance's pairs (the lower job of each)
            out.counts  = c.take<uint32_t>( JobLists::count_at( JOB_LIST_COUNT ) );          // the lists' lengths, a 128-byte line each
            out.class_b = c.take<uint32_t>( classes ? b.n : 1u );                            // the DP's class B, class A and their redo list
            out.class_a = c.take<uint32_t>( classes ? b.n : 1u );
            out.redo    = c.take<uint32_t>( classes ? b.n : 1u );
        } ) );
        // the jobs a chance can still settle, each list through its own launch; every job ends as 0 or 1.
        //   out.second: need_dp == 3, the second chance.
        //   out.third:  the gap chance's jobs -- need_dp == 4 (no diagonal in reach of the other chances: reads with an indel, mostly) and
        //               need_dp == 2 (third-chance jobs: the gap chance evaluates what the third chance only rules out, with the job's best diagonal as
        //               one more class) -- or, without the gap chance (qualities, NVBIO_ALN_NO_GAP_CHANCE), need_dp == 2 for the third chance.
        //   out.pairs:  two need_dp == 4 jobs that are partners (gap_pair_role) as ONE entry, the lower job's id; neither is on out.third.
        //               The gap chance's launch takes them with out.third (NVBIO_ALN_NO_PAIRED_GAP_CHANCE: the first pass makes no pairs).
        // A flag whose launch does not follow (NVBIO_ALN_NO_THIRD_CHANCE: 2; neither launch: none at all) is not in the mask: the first pass hands
        // those jobs to the DP.  (NVBIO_ALN_NO_SECOND_CHANCE keeps the first pass from flagging any 3.)
        const bool gapc = !by_quality && !(b.algo & NVBIO_ALN_NO_GAP_CHANCE);
        const uint32_t third_mask = gapc ? ((third ? 1u << 2 : 0u) | 1u << 4) : (third ? 1u << 2 : 0u);
        // both chances on: ONE launch with the two roles interleaved (chances_e2e31_kernel); NVBIO_ALN_SPLIT_CHANCES keeps them apart (A/B)
        const bool fused = gapc && third && !(b.algo & (NVBIO_ALN_NO_SECOND_CHANCE | NVBIO_ALN_SPLIT_CHANCES));
        const GapLadder lad = gap_ladder( P, G, sc.pat_go, sc.pat_ge );
        NVB_HIP( hipMemsetAsync( out.counts, 0, JobLists::count_at( JOB_LIST_COUNT ) * sizeof(uint32_t), s ) );
        NVB_CHECK( launch_ungapped_e2e31( rbits, 0, by_quality, b, sc, P, G, scores, sinks, need_dp, out, third_mask, nr, s ) );
        if (!fused)     NVB_CHECK( launch_ungapped_e2e31( rbits, 1, false, b, sc, P, G, scores, sinks, need_dp, out, 0u, nr, s ) );
        if (gapc)       NVB_CHECK( launch_gap_chance_e2e31( rbits, fused, b, sc, P, G, lad, scores, sinks, need_dp, out, s ) );
        else if (third) NVB_CHECK( launch_ungapped_e2e31( rbits, 2, false, b, sc, P, G, scores, sinks, need_dp, out, 0u, nr, s ) );
        const uint32_t* jl = out.dp; const uint32_t* jc = out.count( JOB_DP ); ScratchBlock sorted;
        if (sorted_lengths) NVB_CHECK( sort_jobs_by_length( b, out.dp, out.count( JOB_DP ), &jl, &jc, &sorted, s ) );
        if (classes)
        {
            // one launch over the full list, class B and class A; behind it the full band over the (nearly always empty) redo list
            const NarrowJobs nj = { out.class_b, out.count( JOB_CLASS_B ), out.class_a, out.count( JOB_CLASS_A ), out.redo, out.count( JOB_REDO ) };
            NVB_CHECK( launch_pk_kernel( type, rbits, b, sc, pairs, scores, sinks, jl, jc, s, &nj ) );
            NVB_CHECK( launch_pk_kernel( type, rbits, b, sc, pairs, scores, sinks, out.redo, out.count( JOB_REDO ), s ) );
        }
        else
            NVB_CHECK( launch_pk_kernel( type, rbits, b, sc, pairs, scores, sinks, jl, jc, s ) );
        if (routes)
        {
            const dim3 rgrid( (b.n + 255u) / 256u < 4096u ? (b.n + 255u) / 256u : 4096u ), block( 256 );
            NVB_HIP( hipMemsetAsync( routes, 0, b.n, s ) );
            NVB_CHECK( NVB_LAUNCH( job_routes_kernel<false>, rgrid, block, s, out, b.n, classes, routes ) );
            NVB_CHECK( NVB_LAUNCH( job_routes_kernel<true>,  rgrid, block, s, out, b.n, classes, routes ) );
        }
        return NVBIO_OK;
    }
    if (sorted_lengths && b.n > 1u)
    {
        const uint32_t* jl = nullptr; const uint32_t* jc = nullptr; ScratchBlock sorted;
        NVB_CHECK( sort_jobs_by_length( b, nullptr, nullptr, &jl, &jc, &sorted, s ) );
        return launch_pk_kernel( type, rbits, b, sc, pairs, scores, sinks, jl, jc, s );
    }
    return launch_pk_kernel( type, rbits, b, sc, pairs, scores, sinks, nullptr, nullptr, s );
}

} // namespace nvbio_amd
