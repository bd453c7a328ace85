// gotoh_traceback_common.h -- what the banded (gotoh_traceback.hip) and the full-matrix (gotoh_full_traceback.hip) traceback share:
// the direction nibbles, the CIGAR writer, the tails of a job that is not traced or is traced along its diagonal, and the host-side
// scheme checks.  The two DP kernels and the two state walks stay apart: their index spaces and tie rules differ.
#pragma once
#include "gotoh_common.h"

namespace nvbio_amd {

// DirectionVector encodings (nvbio/alignment/alignment.h:326-346): the H move in bits 0-1, the E / F extension flags above
enum : uint32_t { D_SUB = 0u, D_INS = 1u, D_DEL = 2u, D_SINK = 3u, D_INS_EXT = 4u, D_DEL_EXT = 8u };

// A job's CIGAR row, written back to front as nvBowtie's Backtracker does (alignment_utils.h:115-157): elements are type | len << 2
// (io::Cigar; 3 = soft clip).  Elements beyond the row's `stride` are counted, not written: length() > stride marks a truncated row.
struct CigarWriter
{
    uint16_t* cig; uint32_t stride, clen, prev, run;
    __device__ __forceinline__ CigarWriter(uint16_t* cigars, const uint32_t cigar_stride, const uint32_t job)
        : cig( cigars + (size_t)job * cigar_stride ), stride( cigar_stride ), clen( 0 ), prev( 255u ), run( 0 ) {}
    __device__ __forceinline__ void emit(const uint32_t type, const uint32_t len)
    {
        if (clen < stride) cig[clen] = (uint16_t)(type | (len << 2));
        ++clen;
    }
    __device__ __forceinline__ void clip(const uint32_t len) { if (len) emit( 3u, len ); }
    // one step of the walk: equal neighbours join a run
    __device__ __forceinline__ void push(const uint32_t op)
    {
        if (op == prev) ++run;
        else { flush(); prev = op; run = 1u; }
    }
    __device__ __forceinline__ void flush() { if (run) emit( prev, run ); run = 0u; }
    __device__ __forceinline__ uint32_t length() const { return clen; }
};

// a job without a traceback: flag 0 = nothing to trace (banded_inl.h:376-379), 0xFFFFFFFF = skipped, it would overrun the scratch
__device__ __forceinline__ void nothing_traced(uint2* sources, uint32_t* cigar_lens, const uint32_t job, const uint32_t flag)
{
    sources[job]    = make_uint2( 0xFFFFFFFFu, 0xFFFFFFFFu );
    cigar_lens[job] = flag;
}

// the traceback of a job whose optimum is the k diagonal steps that end in its sink: clip, k substitutions, clip
__device__ __forceinline__ void write_diagonal_cigar(uint2* sources, uint16_t* cigars, const uint32_t cigar_stride, uint32_t* cigar_lens,
                                                     const uint32_t job, const uint32_t M, const uint2 sink, const uint32_t k)
{
    CigarWriter cw( cigars, cigar_stride, job );
    cw.clip( M - sink.y );
    if (k) cw.emit( D_SUB, k );
    cw.clip( sink.y - k );
    sources[job]    = make_uint2( sink.x - k, sink.y - k );
    cigar_lens[job] = cw.length();
}

// End-to-end, match bonus 0, open_min >= ext_min > 0 the cheapest open / extension penalties: every step of a path scores <= 0, so a path
// that reaches the optimum `best` holds gaps of at most this many symbols in all (none if |best| < open) and stays within as many
// diagonals of the one it ends on
__device__ __forceinline__ int32_t e2e_gap_bound(const int32_t best, const int32_t open_min, const int32_t ext_min)
{
    const int32_t a = -best;
    return a < open_min ? 0 : (a - open_min) / ext_min + 1;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the magnitudes of a Smith-Waterman scheme as a Gotoh one, for the int16 bound below
inline nvbio_gotoh_scheme as_gotoh(const nvbio_sw_scheme& sw)
{
    return nvbio_gotoh_scheme{ sw.match, -sw.mismatch, -sw.mismatch, sw.deletion, sw.deletion, sw.insertion, sw.insertion };
}
// the reference re-derives the direction vectors from int16 checkpoints (clamped at -32736, gotoh_banded_inl.h:216-222); the single
// pass here equals that iff no score of a path over `cells` cells can leave that range
inline bool int16_checkpoints_ok(const nvbio_gotoh_scheme& scheme, const int64_t cells)
{
    return cells * scheme_max_step( scheme_dev( &scheme ) ) <= 30000;
}
// nvBowtie's end-to-end mode, where e2e_gap_bound holds: *go_min / *ge_min are the cheapest open / extension penalties
inline bool narrow_e2e(const SchemeDev& sc, const int type, const uint32_t algo, int32_t* go_min, int32_t* ge_min)
{
    *go_min = -(sc.pat_go > sc.txt_go ? sc.pat_go : sc.txt_go);
    *ge_min = -(sc.pat_ge > sc.txt_ge ? sc.pat_ge : sc.txt_ge);
    return type == NVBIO_SEMI_GLOBAL && sc.match == 0 && sc.mm_min >= 0 && sc.mm_max >= 0 && plain_gotoh( sc ) &&
           *ge_min > 0 && *go_min >= *ge_min && !(algo & NVBIO_ALN_NO_NARROW_TRACEBACK);
}

} // namespace nvbio_amd
