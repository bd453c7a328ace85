// band31_jobs.h -- what the units of the band-31 scoring stage share: the job lists the passes hand jobs on through, the rules that give a
// job its route (narrow classes, the gap chance's ladder and pairs), and the host launchers of each unit's kernels.  The stage, in launch
// order (band31_stage.hip: launch_pk): the first pass over every job (band31_first_pass.hip), the chances over what it could not settle
// (band31_chances.hip), the packed DP over the rest (band31_packed.hip).
#pragma once
#include "gotoh_common.h"
#include "bitplanes.h"

namespace nvbio_amd {

// the gap chance's cost ladder (gap_chance_e2e31_kernel): the cheapest class of gapped alignments it neither evaluates nor rules out, with P the
// least a mismatch can cost and gaps of up to GAP_CHANCE_GA symbols evaluated
constexpr int GAP_CHANCE_GA = 5;
__host__ __device__ __forceinline__ int32_t gap_chance_unknown_cost(const int32_t P, const int32_t go, const int32_t ge)
{
    auto cg = [&](const int g) -> int32_t { return -(go + (g - 1) * ge); };
    int32_t c = cg( 1 ) + 3 * P;                                  // one gap and three mismatches
    const int32_t others[] = { cg( GAP_CHANCE_GA + 1 ), 3 * cg( 1 ), 2 * cg( 1 ) + P, cg( 1 ) + cg( 3 ), 2 * cg( 2 ) };
    #pragma unroll
    for (int k = 0; k < 5; ++k) c = others[k] < c ? others[k] : c;
    return c;
}
// what the gap chance needs of the ladder beyond the kernel's own arguments, computed ONCE on the host (it depends on the scheme only, and
// `cap` is a 64-bit division that every wave used to expand: two v_rcp_f32 and some 160 scalar instructions): c_unk for a job that brings its best diagonal (need_dp = 2)
// and for one that does not (need_dp = 4: every diagonal has more than `cap` mismatches, so the ungapped class costs >= (cap + 1) P)
struct GapLadder { int32_t c_unk_u, c_unk_n; };
constexpr int NARROW_A_HALF = 6, NARROW_B_HALF = 8;              // half-widths of class A / B around column 15
struct NarrowJobs { const uint32_t *list_b, *count_b, *list_a, *count_a; uint32_t *redo, *redo_count; };
// the DP's narrow classes (banded_gotoh_band31_pk_kernel, NARROW), decided by the first pass from U* and the best diagonal alone: with
// r(L) = the largest delta with open + (delta - 1) ext >= L and w = r(U*) + |best_d - 15|, class A is w <= NARROW_A_HALF, class B
// w <= NARROW_B_HALF.  The host passes thr_a / thr_b = the least U* with r <= the half-width, open + half ext + 1 (they depend on the scheme
// only); a window off centre by o columns raises them by -o ext.  thr = 1, which no U* reaches: the route is off.  A class comes out empty by
// itself for a scheme whose U* of the jobs that leave for the DP all lie below its threshold (cheap gaps: the threshold is close to 0).
// cnt_max: the first pass counts a diagonal's mismatches exactly up to the larger of its own cap and this, the largest count whose U* is
// still in class B, so that a job whose best diagonal is out of every chance's reach leaves with its U* known.
struct NarrowRule { int32_t thr_a, thr_b; uint32_t cnt_max; };
// 0: none, 1: class B, 2: class A
__device__ __forceinline__ uint32_t narrow_class(const NarrowRule nr, const int64_t U, const uint32_t best_d, const int32_t gap_ext)
{
    const int64_t o = best_d > 15u ? best_d - 15u : 15u - best_d;
    if (o <= NARROW_A_HALF && U >= (int64_t)nr.thr_a - o * gap_ext) return 2u;
    if (o <= NARROW_B_HALF && U >= (int64_t)nr.thr_b - o * gap_ext) return 1u;
    return 0u;
}

// ---- the stage's job lists, appended to by the kernels that decide a job's route ----
// Each kernel in front of the DP holds a job's flag in a register when it stores need_dp[job]; it puts the job id on the list of the launch
// that takes the job next itself.  Per workgroup and list: the waves count their jobs with a ballot, ONE lane reserves the workgroup's range
// with a returning atomicAdd on the list's counter (none when the workgroup has no job for the list), every lane stores its id at the
// range's start + the jobs of the waves before it + its rank in the ballot.  A workgroup walks JOB_LIST_CHUNKS chunks of 256 jobs and
// reserves once for all of them.  The lists are dense but NOT in ascending job order (workgroups reserve in the order they finish).
// Counters: `counts` of the "banded_job_list" layout, one 128-byte line each, zeroed on the stream before the first pass.
enum JobList : uint32_t
{
    JOB_DP,                                                       // the DP's full list
    JOB_SECOND,                                                   // the second chance's
    JOB_THIRD,                                                    // the third / gap chance's
    JOB_PAIRS,                                                    // the gap chance's pairs
    JOB_CLASS_B, JOB_CLASS_A,                                     // the DP's narrow roles (narrow_class() = 1, 2)
    JOB_REDO,                                                     // the narrow roles' redo list
    JOB_LIST_COUNT
};
static_assert( JOB_CLASS_A == JOB_CLASS_B + 1, "narrow_class() 1, 2 = class B, class A, in this order" );
constexpr uint32_t JOB_COUNT_STRIDE = 32u;                        // in uint32: a 128-byte line per counter
#ifndef NVB_JOB_LIST_CHUNKS
#define NVB_JOB_LIST_CHUNKS 1
#endif
constexpr int JOB_LIST_CHUNKS = NVB_JOB_LIST_CHUNKS;              // at most 4 (JobAppend::mine holds a byte per chunk for up to 3 lists, 16 bits per chunk in a uint64_t beyond)
static inline uint32_t job_list_grid(const uint32_t n) { return (n + 256u * JOB_LIST_CHUNKS - 1u) / (256u * JOB_LIST_CHUNKS); }

struct JobLists
{
    uint32_t *dp, *second, *third, *pairs; uint32_t* counts; uint32_t *class_b, *class_a, *redo;      // the lists in JobList's order, and the counters
    // where list's counter lies in `counts`, in uint32 (list = JOB_LIST_COUNT: the uint32 `counts` holds), and the counter itself
    static __host__ __device__ constexpr uint32_t count_at(const uint32_t list) { return JOB_COUNT_STRIDE * list; }
    __host__ __device__ __forceinline__ uint32_t* count(const uint32_t list) const { return counts + count_at( list ); }
};

template <int NL>
struct JobAppend
{
    static_assert( NL >= 1 && NL <= 6 && JOB_LIST_CHUNKS >= 1 && JOB_LIST_CHUNKS <= 4, "JobAppend: up to 6 lists, up to 4 chunks" );
    struct Lds { uint32_t cnt[NL][4 * JOB_LIST_CHUNKS]; uint32_t base[NL]; };
    // chunk k in bits SLOT k .. SLOT k + SLOT - 1: (list + 1) << 6 | rank among the wave's jobs for that list (a byte holds lists 0 .. 2)
    static constexpr int SLOT = NL <= 3 ? 8 : 16;
    typedef typename std::conditional<NL <= 3, uint32_t, uint64_t>::type Mine;
    Mine mine = 0;
    // chunk k's job of this lane goes on list `which` (-1: on none).  Called by EVERY lane of the workgroup (256 threads), converged.
    __device__ __forceinline__ void note(Lds& lds, const int k, const int which)
    {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        #pragma unroll
        for (int l = 0; l < NL; ++l)
        {
            const uint64_t m = __ballot( which == l );
            if (lane == 0) lds.cnt[l][4 * k + wave] = (uint32_t)__popcll( m );
            if (which == l) mine |= (Mine)(((uint32_t)(l + 1) << 6) | (uint32_t)__popcll( m & ((1ull << lane) - 1ull) )) << (SLOT * k);
        }
    }
    // reserve and store; job_of( k ) = the id of this lane's job of chunk k.  Called once by every lane of the workgroup, after the last note().
    template <typename JobOf>
    __device__ __forceinline__ void flush(Lds& lds, const JobLists& out, JobOf job_of)
    {
        __syncthreads();
        if (threadIdx.x < (uint32_t)NL)
        {
            uint32_t tot = 0;
            for (int i = 0; i < 4 * JOB_LIST_CHUNKS; ++i) { const uint32_t c = lds.cnt[threadIdx.x][i]; lds.cnt[threadIdx.x][i] = tot; tot += c; }
            lds.base[threadIdx.x] = tot ? atomicAdd( out.count( threadIdx.x ), (unsigned int)tot ) : 0u;
        }
        __syncthreads();
        const uint32_t wave = threadIdx.x >> 6;
        #pragma unroll
        for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
        {
            const uint32_t e = (uint32_t)(mine >> (SLOT * k)) & ((1u << SLOT) - 1u);
            if (e)
            {
                const uint32_t l = (e >> 6) - 1u;
                uint32_t* const list = l == JOB_DP ? out.dp : (l == JOB_SECOND ? out.second : (l == JOB_THIRD ? out.third : (l == JOB_PAIRS ? out.pairs : (l == JOB_CLASS_B ? out.class_b : out.class_a))));
                list[lds.base[l] + lds.cnt[l][4 * k + wave] + (e & 63u)] = job_of( k );
            }
        }
    }
};

// the same for a kernel whose lanes hold TWO jobs each (a pair of the gap chance) and put either, both or none on out.dp: one ballot round per
// member, one reservation per workgroup
struct JobAppendTwo
{
    struct Lds { uint32_t cnt[2 * 4 * JOB_LIST_CHUNKS]; uint32_t base; };
    uint64_t mine = 0;                                            // chunk k, member r in bits 16k + 8r .. + 7: 64 | rank among the wave's jobs of that round
    __device__ __forceinline__ void note(Lds& lds, const int k, const bool first, const bool second)
    {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        #pragma unroll
        for (int r = 0; r < 2; ++r)
        {
            const bool on = r ? second : first;
            const uint64_t m = __ballot( on );
            if (lane == 0) lds.cnt[4 * (2 * k + r) + wave] = (uint32_t)__popcll( m );
            if (on) mine |= (uint64_t)(64u | (uint32_t)__popcll( m & ((1ull << lane) - 1ull) )) << (16 * k + 8 * r);
        }
    }
    // job_of( k, r ) = the id of member r of this lane's pair of chunk k
    template <typename JobOf>
    __device__ __forceinline__ void flush(Lds& lds, const JobLists& out, JobOf job_of)
    {
        __syncthreads();
        if (threadIdx.x == 0)
        {
            uint32_t tot = 0;
            for (int i = 0; i < 2 * 4 * JOB_LIST_CHUNKS; ++i) { const uint32_t c = lds.cnt[i]; lds.cnt[i] = tot; tot += c; }
            lds.base = tot ? atomicAdd( out.count( JOB_DP ), (unsigned int)tot ) : 0u;
        }
        __syncthreads();
        const uint32_t wave = threadIdx.x >> 6;
        #pragma unroll
        for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
            #pragma unroll
            for (int r = 0; r < 2; ++r)
            {
                const uint32_t e = (uint32_t)(mine >> (16 * k + 8 * r)) & 255u;
                if (e) out.dp[lds.base + lds.cnt[4 * (2 * k + r) + wave] + (e & 63u)] = job_of( k, r );
            }
    }
};

// ---- the gap chance's pairs ----
// A read with an indel has exact seeds on two diagonals a few columns apart and reaches this stage as two candidates whose band-31 windows
// overlap in all but those few columns: 31 - shift of either job's 31 diagonals are the same diagonals of the same read against the same
// text.  Two such jobs that the first pass BOTH sends to the gap chance go there as one entry (list `pairs`), and gap_chance_e2e31_pair walks
// the 31 + shift diagonals once for the two.  Which jobs may pair is a function of the batch's geometry alone (nvbio_banded_gap_pairs
// reports it): jobs j and j + 1 are linked iff they have the same read and flags, unclipped windows of read length + 31 symbols and
// 0 < |win_begin[j+1] - win_begin[j]| <= PAIR_MAX_SHIFT, and lie in the same wave of the first pass (64 consecutive jobs); a run of linked
// jobs pairs up from its lowest job.  Nothing is sorted to make candidates adjacent: the seed pass hands a read's candidates over together,
// strand by strand, in SEED order with equal neighbours dropped (emit_seed_results) -- contiguous, but not ascending in diagonal: a read
// with an insertion (or a deletion on the other strand) brings its higher diagonal first -- so the rule takes either order of win_begin.
// PAIR_MAX_SHIFT = 5 covers every gap the gap chance evaluates; the union window then has up to 161 + 31 + 5 = 197 symbols: 14 packed text
// words (209 symbols at any storage offset) where the single job loads 13.
constexpr uint32_t PAIR_MAX_SHIFT = NVBIO_GAP_PAIR_MAX_SHIFT;

// +1: `job` is the lower job of a pair (its partner is job + 1), -1: the upper one, 0: neither.  Called by all 64 lanes of a wave whose lane l
// holds job (job of lane 0) + l; live = the lane has a job at all
__device__ __forceinline__ int gap_pair_role(const BatchDev& b, const uint32_t job, const bool live)
{
    uint32_t rid = 0, fl = 0, tb = 0, whole = 0;
    if (live)
    {
        rid = b.read_id ? b.read_id[job] : job;
        const uint32_t M = b.read_offsets[rid + 1] - b.read_offsets[rid];
        fl = b.flags ? b.flags[job] : 0u;
        tb = b.win_begin[job];
        whole = (M >= 1u && M <= PLANE_MAX_READ && b.win_end[job] - tb == M + 31u) ? 1u : 0u;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rid_n = __shfl_down( rid, 1 ), fl_n = __shfl_down( fl, 1 ), tb_n = __shfl_down( tb, 1 ), whole_n = __shfl_down( whole, 1 );
    const uint32_t shift = tb_n > tb ? tb_n - tb : tb - tb_n;      // (either job may hold the lower window)
    const bool link = lane < 63u && whole && whole_n && rid_n == rid && fl_n == fl && shift >= 1u && shift <= PAIR_MAX_SHIFT;
    const uint64_t links = __ballot( link );
    const uint32_t run = lane ? (uint32_t)__clzll( (long long)~(links << (64u - lane)) ) : 0u;     // linked lanes right below this one
    const bool lower = link && !(run & 1u);
    const uint64_t lowers = __ballot( lower );
    if (lower) return 1;
    return (lane && ((lowers >> (lane - 1u)) & 1ull)) ? -1 : 0;
}

// ---- the units' host launchers: each enqueues its unit's kernel for the read bits (4 or 2) and, where given, the alignment type ----
// band31_packed.hip: the packed DP.  packed_ok: the 16-bit lanes are exact for this scheme; pk_binary16_ok: so are binary16 lanes;
// launch_pk_kernel: over job_list (NULL: every job of the batch), `pairs` lanes; narrow: with the lists of the narrow roles
bool packed_ok(const int type, const SchemeDev& sc, const uint32_t max_read_len);
bool pk_binary16_ok(const int type, const BatchDev& b, const SchemeDev& sc);
nvbio_status launch_pk_kernel(const int type, const uint32_t rbits, const BatchDev& b, const SchemeDev& sc, const uint32_t pairs, int32_t* scores, uint2* sinks,
                              const uint32_t* job_list, const uint32_t* job_count, hipStream_t s, const NarrowJobs* narrow = nullptr);
// band31_first_pass.hip: ungapped_e2e31_kernel<rbits, mode, by_quality> (by_quality: mode 0 only); mode 0 over every job, mode 1 / 2 over
// out.second / out.third
nvbio_status launch_ungapped_e2e31(const uint32_t rbits, const int mode, const bool by_quality, const BatchDev& b, const SchemeDev& sc, const int32_t P,
                                   const int32_t G, int32_t* scores, uint2* sinks, uint8_t* need_dp, const JobLists& out, const uint32_t third_mask,
                                   const NarrowRule nr, hipStream_t s);
// band31_chances.hip: the gap chance over out.third and out.pairs (gap_chance_e2e31_kernel) or, with_second, both chances in one launch,
// over out.second too (chances_e2e31_kernel); and the pairs' report of nvbio_banded_gap_pairs
nvbio_status launch_gap_chance_e2e31(const uint32_t rbits, const bool with_second, const BatchDev& b, const SchemeDev& sc, const int32_t P, const int32_t G,
                                     const GapLadder lad, int32_t* scores, uint2* sinks, uint8_t* need_dp, const JobLists& out, hipStream_t s);
nvbio_status launch_gap_pairs(const BatchDev& b, uint32_t* partner, hipStream_t s);
// band31_stage.hip: the whole stage; routes: the route report of nvbio_banded_gotoh_score_routes (NULL: none), preset to 1 by the caller
nvbio_status launch_pk(const int type, const uint32_t rbits, const BatchDev& b, const SchemeDev& sc, int32_t* scores, uint2* sinks, hipStream_t s, uint8_t* routes);

// the read widths the stage is instantiated for (the text: 2 bits).  (In this order: the compiler instantiates a dispatcher's last entry first,
// and chances_e2e31_kernel compiles to the code profiles/band31_split_resource_usage.txt records only with its 4-bit build ahead of its 2-bit one.
// Reordering this list, or the launchers' use of it, changes that kernel's code though no kernel's text changes: after touching either, run
// scripts/resource_report.py again and hold it against that file.)
using ReadBits31 = Values<2, 4>;

} // namespace nvbio_amd
