// band31_first_pass.hip -- the band-31 end-to-end first pass (ungapped_e2e31_job over every job of the batch) and its list passes
// (the second and the third chance as launches of their own), for gfx950.
#include "band31_ungapped_inl.h"

namespace nvbio_amd {

// MODE 0: every job of the batch; its flag goes to need_dp (the gap chance tells 2 from 4 by it) and its id on the list of the launch that
//   takes it next: flag 3 on out.second, a flag in `third_mask` (bit f set: flag f is taken by the launch over out.third -- the host passes
//   the flags of the launch that really follows, none when none does) on out.third, any other non-zero flag on out.dp.
// MODE 1 / 2: the jobs of job_list; one that ends as 1 goes on out.dp.  (Launched over the whole batch's workgroups: those behind the
//   list's end leave before they touch anything.)
template <int RBITS, int MODE, bool QUAL = false>
// (the first pass proper keeps its 7 waves per SIMD, i.e. 72 registers: left alone the allocator takes 73 on the route over the text's planes.
// Under a forced minimum a job that outgrows the budget SPILLS instead of losing a wave, and nothing says so at build time: after any edit of
// band31_ungapped_inl.h or of what it includes, run scripts/resource_report.py again and hold it against profiles/band31_split_resource_usage.txt --
// scratch 0, spills 0 for every instantiation.  The (1) of the other instantiations asks for nothing: their figures are the parent's.)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MODE == 0 && !QUAL) ? 7 : 1)))
ungapped_e2e31_kernel(const BatchDev b, const int32_t P, const int32_t G, const int32_t gap_open, const int32_t gap_ext,
                      int32_t* __restrict__ scores, uint2* __restrict__ sinks, uint8_t* __restrict__ need_dp,
                      const uint32_t* __restrict__ job_list, const uint32_t* __restrict__ job_count,
                      const SchemeDev sc, const JobLists out, const uint32_t third_mask, const NarrowRule nr)
{
    constexpr bool LIST = MODE != 0;
    constexpr int  NL   = LIST ? 1 : 6;
    __shared__ int32_t s_pen[QUAL ? 64 : 1];
    __shared__ typename JobAppend<NL>::Lds s_lists;
    const uint32_t n    = LIST ? *job_count : b.n;
    const uint32_t slot0 = blockIdx.x * (256u * JOB_LIST_CHUNKS);
    if (slot0 >= n) return;                                          // (the whole workgroup)
    if (QUAL)
    {
        if (threadIdx.x < 64) s_pen[threadIdx.x] = -mismatch_score( sc, threadIdx.x );     // the DP kernels' table, negated
        __syncthreads();
    }
    JobAppend<NL> app;
    auto job_of = [&](const int k) -> uint32_t { const uint32_t slot = slot0 + 256u * k + threadIdx.x; return LIST ? job_list[slot] : slot; };
    // (flag 4 goes to the gap chance at all; batches declared ragged keep the stage they had: single jobs only)
    const bool pairing = ((third_mask >> 4) & 1u) && !(b.algo & (NVBIO_ALN_NO_PAIRED_GAP_CHANCE | NVBIO_ALN_RAGGED_READS));
    #pragma unroll 1
    for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
    {
        int which = -1;
        uint32_t flag = 0;
        if (slot0 + 256u * k + threadIdx.x < n)
        {
            const uint32_t job  = job_of( k );
            flag = ungapped_e2e31_job<RBITS,MODE,QUAL>( b, P, G, gap_open, gap_ext, scores, sinks, job, s_pen, nr );
            const uint32_t cls = flag >> 8;                          // (MODE 0: a flag-1 job's narrow class, 1 = B on JOB_CLASS_B, 2 = A on JOB_CLASS_A)
            flag &= 255u;
            need_dp[job] = (uint8_t)flag;
            if (flag) which = LIST ? JOB_DP : (flag == 3u ? JOB_SECOND : (((third_mask >> flag) & 1u) ? JOB_THIRD : (cls ? JOB_CLASS_B - 1 + (int)cls : JOB_DP)));
        }
        if (MODE == 0 && !QUAL && pairing && __any( flag == 4u ))
        {
            // two partners (gap_pair_role) that BOTH go to the gap chance go as one entry of list `pairs`, put there by the lower one
            const uint32_t slot = slot0 + 256u * k + threadIdx.x;
            const int role = gap_pair_role( b, slot, slot < n );
            const uint32_t flag_up = __shfl_down( flag, 1 ), flag_dn = __shfl_up( flag, 1 );
            if (role > 0 && flag == 4u && flag_up == 4u) which = JOB_PAIRS;
            if (role < 0 && flag == 4u && flag_dn == 4u) which = -1;
        }
        app.note( s_lists, k, which );
    }
    app.flush( s_lists, out, job_of );
}

nvbio_status launch_ungapped_e2e31(const uint32_t rbits, const int mode, const bool by_quality, const BatchDev& b, const SchemeDev& sc, const int32_t P,
                                   const int32_t G, int32_t* scores, uint2* sinks, uint8_t* need_dp, const JobLists& out, const uint32_t third_mask,
                                   const NarrowRule nr, hipStream_t s)
{
    const dim3 grid( job_list_grid( b.n ) ), block( 256 );
    const uint32_t* job_list  = mode == 1 ? out.second : (mode == 2 ? out.third : nullptr);
    const uint32_t* job_count = mode == 1 ? out.count( JOB_SECOND ) : (mode == 2 ? out.count( JOB_THIRD ) : nullptr);
    auto miss = [&] { set_error( "band-31 first pass: read_bits %u, mode %d not instantiated", rbits, mode ); return NVBIO_ERR_UNSUPPORTED; };
    return with_value( ReadBits31(), (int)rbits, [&](auto RB)
    {
        if (by_quality && mode == 0)
            return NVB_LAUNCH( (ungapped_e2e31_kernel<RB,0,true>), grid, block, s, b, P, G, sc.pat_go, sc.pat_ge, scores, sinks, need_dp, job_list, job_count,
                               sc, out, third_mask, nr );
        return with_value( Values<0, 1, 2>(), by_quality ? -1 : mode, [&](auto MODE)
        {
            // (the list passes take neither a quality ramp nor routes of their own)
            return NVB_LAUNCH( (ungapped_e2e31_kernel<RB,MODE>), grid, block, s, b, P, G, sc.pat_go, sc.pat_ge, scores, sinks, need_dp, job_list, job_count,
                               MODE == 0 ? sc : SchemeDev{}, out, MODE == 0 ? third_mask : 0u, MODE == 0 ? nr : NarrowRule{ 1, 1, 0u } );
        }, miss );
    }, miss );
}

} // namespace nvbio_amd
