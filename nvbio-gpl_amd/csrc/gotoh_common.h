// gotoh_common.h -- types shared by the banded and full-matrix Gotoh kernels.
#pragma once
#include "common.h"

namespace nvbio_amd {

// flattened stream of alignment jobs (see nvbio_alignment_batch)
struct BatchDev
{
    const void*     reads;
    const uint32_t* read_offsets;
    const uint8_t*  quals;
    const uint32_t* read_id;
    const uint8_t*  flags;
    const void*     text;
    const uint32_t* win_begin;
    const uint32_t* win_end;
    uint32_t        n;
    uint32_t        max_read_len;
    uint32_t        algo;              // NVBIO_ALN_* (host-side kernel selection only)
    const void*     text_planes;       // the text as bit planes (bitplanes.h: load_text_units), or NULL: the packed words are converted per job
};

// Scoring scheme as the kernels see it.  The reference's Gotoh kernels take BOTH gap recurrences from the pattern-gap terms and
// use the text-gap terms only to initialise the boundaries (gotoh_banded_inl.h:435-439,48; gotoh_inl.h:641-642,69-70); its
// linear-gap Smith-Waterman kernels charge `deletion` where the text advances alone and `insertion` where the pattern does, in
// the recurrences and on the boundaries alike (sw/sw_banded_inl.h:369-370,44; sw/sw_inl.h:69-70,628-629,650).  Both fit:
//   pat_go/pat_ge : the gap that consumes text only   (banded: F, from band j+1; full: along the text)
//   ins_go/ins_ge : the gap that consumes pattern only (banded: E, along the band; full: along the pattern)
//   txt_go/txt_ge : boundary that is read first (banded row zero, the full matrix's boundary column)
//   top_go/top_ge : the full matrix's stripe-top boundary
//   wide          : full matrix swept in logical stripes of 16 (sw_bandlen_selector, sw/sw_inl.h:1322-1325) instead of 8: it
//                   decides LOCAL ties between cells of equal score and where the early exit is tested
struct SchemeDev
{
    int32_t match, mm_min, mm_max, pat_go, pat_ge, txt_go, txt_ge;
    int32_t ins_go, ins_ge, top_go, top_ge, wide;
};

inline SchemeDev scheme_dev(const nvbio_gotoh_scheme* g)
{
    return SchemeDev{ g->match, g->mm_min, g->mm_max, g->pat_gap_open, g->pat_gap_ext, g->txt_gap_open, g->txt_gap_ext,
                      g->pat_gap_open, g->pat_gap_ext, g->pat_gap_open, g->pat_gap_ext, 0 };
}
// boundary_over_pattern: the first-read boundary runs along the pattern (full matrix, text blocking) instead of the text
inline SchemeDev scheme_dev(const nvbio_sw_scheme* w, const bool boundary_over_pattern)
{
    const int32_t D = w->deletion, I = w->insertion;
    const int32_t b = boundary_over_pattern ? I : D, t = boundary_over_pattern ? D : I;
    return SchemeDev{ w->match, -w->mismatch, -w->mismatch, D, D, b, b, I, I, t, t, 1 };
}
// true when the scheme is an ordinary reference-Gotoh one (what the packed kernels and the ungapped shortcuts assume)
inline bool plain_gotoh(const SchemeDev& sc)
{
    return !sc.wide && sc.ins_go == sc.pat_go && sc.ins_ge == sc.pat_ge && sc.top_go == sc.pat_go && sc.top_ge == sc.pat_ge;
}

// What the alignment kernels are instantiated for (common.h: with_value, with_bits)
using AlnTypes   = Values<NVBIO_GLOBAL, NVBIO_LOCAL, NVBIO_SEMI_GLOBAL>;
using Bands      = Values<3, 7, 15, 31>;
using BitsAll    = BitsList<Bits<4,2>, Bits<2,2>, Bits<8,2>, Bits<8,8>, Bits<4,8>, Bits<2,8>>;     // every pair make_batch accepts
using BitsBest2  = BitsList<Bits<4,2>, Bits<2,2>, Bits<8,2>, Bits<8,8>>;                           // Best2Sink scorers, Myers
using BitsStaged = BitsList<Bits<4,2>, Bits<2,2>, Bits<8,8>>;                                      // the staged scorer

// the band check of the banded entry points: `bad` is what a band outside Bands gets -- UNSUPPORTED from the scorers, INVALID from the
// tracebacks
inline nvbio_status check_band(const uint32_t band, const nvbio_status bad)
{
    if (with_value( Bands(), (int)band, [](auto) { return true; }, [] { return false; } )) return NVBIO_OK;
    if (bad == NVBIO_ERR_UNSUPPORTED) set_error( "band %u is not instantiated (3, 7, 15, 31)", band );
    else                              set_error( "invalid argument: band must be 3, 7, 15 or 31" );
    return bad;
}

// what an alignment type outside AlnTypes gets
inline nvbio_status invalid_type(const int type)
{
    set_error( "invalid alignment type %d", type );
    return NVBIO_ERR_INVALID;
}
// what a (read_bits, text_bits) pair outside BitsAll gets
inline nvbio_status invalid_bits(const uint32_t rbits, const uint32_t tbits)
{
    set_error( "unsupported read_bits/text_bits %u/%u", rbits, tbits );
    return NVBIO_ERR_INVALID;
}

nvbio_status make_batch(const nvbio_alignment_batch* in, BatchDev* b);      // gotoh_banded.hip
nvbio_status banded15_full_ties_traceback(const BatchDev& b, const SchemeDev& sc, const uint32_t rbits, const uint32_t tbits, const uint32_t max_jobs,
                                          const uint32_t* job_list, const uint32_t* job_count, uint32_t* dirs, const uint64_t dirs_bytes,
                                          int32_t* scores, uint2* sources, uint2* sinks, uint16_t* cigars, const uint32_t stride, uint32_t* lens,
                                          hipStream_t s);                   // gotoh_traceback.hip
bool banded31_packed_ok(const SchemeDev& sc, const uint32_t max_read_len);  // band31_packed.hip
nvbio_status banded31_packed_launch(const BatchDev& b, const SchemeDev& sc, const uint32_t read_bits, const uint32_t max_jobs, int32_t* scores, uint2* sinks,
                                    const uint32_t* job_list, const uint32_t* job_count, hipStream_t s);

// QualCost (nvBowtie/bowtie2/cuda/scoring.h:84-88) negated (:280-281); IEEE float ops, no contraction
__device__ __forceinline__ int32_t mismatch_score(const SchemeDev& sc, const uint32_t q)
{
    const int   qi   = (int)q < 40 ? (int)q : 40;
    const float frac = (float)qi / 40.0f;
    return -( sc.mm_min + (int)( frac * (float)(sc.mm_max - sc.mm_min) ) );
}

__device__ __forceinline__ int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
__device__ __forceinline__ int32_t max3(int32_t a, int32_t b, int32_t c) { return max2( max2( a, b ), c ); }

// the largest magnitude of a single step of the scheme: what the int16 / binary16 range checks of the host multiply by the path length.
// (The Smith-Waterman aligner's terms enter through scheme_dev / as_gotoh.)
inline int64_t scheme_max_step(const SchemeDev& sc)
{
    int64_t step = 0;
    const int64_t c[] = { sc.match, sc.mm_min, sc.mm_max, sc.pat_go, sc.pat_ge, sc.txt_go, sc.txt_ge };
    for (int64_t v : c) { if (v < 0) v = -v; if (v > step) step = v; }
    return step;
}

// launches over `n` slots, at most `cap` per launch: f( begin, jobs ) until one fails
template <typename F>
inline nvbio_status for_each_chunk(const uint64_t n, const uint64_t cap, F f)
{
    nvbio_status st = NVBIO_OK;
    for (uint64_t begin = 0; begin < n && st == NVBIO_OK; begin += cap)
        st = f( (uint32_t)begin, (uint32_t)((n - begin) < cap ? (n - begin) : cap) );
    return st;
}

// ---- the job as the kernels see it --------------------------------------------------------------------------------------------------
// pattern = symbols [first, first + M) of the read stream, read backwards (rev) and complemented (comp) as the job's flag byte `fl` says;
// text = the N symbols from tb on, N as the window stores it
struct AlnJob
{
    uint32_t first, M, tb, N, fl; bool rev, comp;
};
__device__ __forceinline__ uint32_t read_len(const BatchDev& b, const uint32_t job)
{
    const uint32_t rid = b.read_id ? b.read_id[job] : job;
    return b.read_offsets[rid + 1] - b.read_offsets[rid];
}
__device__ __forceinline__ AlnJob load_job(const BatchDev& b, const uint32_t job)
{
    AlnJob j;
    const uint32_t rid = b.read_id ? b.read_id[job] : job;
    j.first = b.read_offsets[rid];
    j.M     = b.read_offsets[rid + 1] - j.first;
    j.fl    = b.flags ? b.flags[job] : 0u;
    j.rev   = (j.fl & NVBIO_READ_REVERSE) != 0;
    j.comp  = (j.fl & NVBIO_READ_COMPLEMENT) != 0;
    j.tb    = b.win_begin[job];
    j.N     = b.win_end[job] - j.tb;
    return j;
}
// The scorers' rule: a pattern longer than the batch's declared max_read_len is rejected -- nothing reported, as for a text shorter than
// the pattern -- in every scoring kernel alike: the packed kernels rely on that bound for their 16-bit scores.  (The tracebacks keep N
// and flag such a job with cigar_lens = 0xFFFFFFFF; the full-matrix scorer is bounded by its max_M / max_N instead.)
__device__ __forceinline__ uint32_t scored_text_len(const BatchDev& b, const AlnJob& J)
{
    return (b.max_read_len && J.M > b.max_read_len) ? 0u : J.N;
}

// row i of the pattern: its symbol as the DP compares it, and the storage index (of the symbol and of its quality) in *pidx
template <typename Reader>
__device__ __forceinline__ uint32_t pattern_symbol(Reader& prd, const AlnJob& J, const uint32_t i, uint32_t* pidx)
{
    *pidx = J.rev ? J.first + J.M - 1u - i : J.first + i;
    const uint32_t q = prd.get( *pidx );
    return (J.comp && q < 4u) ? 3u - q : q;
}
// the mismatch score of the row stored at pidx, from the workgroup's table (qualities >= 40 all map to mm_max)
__device__ __forceinline__ int32_t pattern_mismatch(const uint8_t* quals, const int32_t* s_mm, const uint32_t pidx)
{
    const uint32_t qq = quals ? quals[pidx] : 0u;
    return s_mm[qq < 63u ? qq : 63u];
}
// mismatch score per quality value, computed once per workgroup into a __shared__ int32_t[64].  Holds a barrier: every thread of the
// workgroup calls it, before any early return.
__device__ __forceinline__ void fill_mismatch_table(int32_t* s_mm, const SchemeDev& sc)
{
    if (threadIdx.x < 64) s_mm[threadIdx.x] = mismatch_score( sc, threadIdx.x );
    __syncthreads();
}

// slot t of a launch over `jobs` slots from job_begin on: with a job list (the jobs an earlier pass could not settle, its length on the
// device) entry job_begin + t of the list, else job job_begin + t.  False where the slot holds no job.
__device__ __forceinline__ bool slot_job(const uint32_t* job_list, const uint32_t* job_count, const uint32_t job_begin, const uint32_t t,
                                         const uint32_t jobs, uint32_t* job)
{
    if (t >= jobs) return false;
    if (job_list && job_begin + t >= *job_count) return false;
    *job = job_list ? job_list[job_begin + t] : job_begin + t;
    return true;
}

} // namespace nvbio_amd
