// sam.hip -- nvBowtie's SAM records, formatted on the device (gfx950):
//         itoa, generate_cigar_string, generate_md_string           nvbio/io/output/output_sam.cpp:76-115,182-212,216-289
//         output_alignment, process_one_alignment                   nvbio/io/output/output_sam.cpp:292-342,344-544
// The reference formats on the host, one fwrite per field and one read after another.  A record's text is a pure function of arrays that
// already sit in HBM, so here it is produced in three steps on the caller's stream: the byte length of every record, an exclusive uint64
// scan of the lengths (a batch can exceed 4 GiB), and the write.
//
// Shape of the two kernels: ONE WAVE PER RECORD, four records per 256-lane workgroup.  The code of a wave is uniform -- the record index
// is a scalar, so the record's header, its CIGAR sums and the walk over its MDS stream are scalar work -- except where lanes stripe: the
// QNAME and RNAME bytes, the CIGAR elements (a wave-wide scan of their text widths places each element), and SEQ and QUAL, about three
// quarters of a record, which each lane unpacks from the 4-bit read one symbol at a time.  The write kernel composes the record in LDS
// at the byte residue (mod 16) its global offset has and then copies it out: byte stores for the unaligned head and tail only, 16-byte
// stores from 16-byte LDS reads for the body.  The length kernel runs the same code with the stores compiled out, so the two cannot
// disagree; the write kernel still compares its own length with the caller's offsets and refuses a record that differs.
//
// Limit: a wave's LDS holds SAM_LDS[k] bytes (at most 16384: four waves share the 64 KiB a workgroup may declare), of which 16 go to the
// residue and mds_stride (rounded up to 16) to the staged MDS stream.  The bound on a record's text is derived on the host:
//   max_name_len + 2 * refs->max_name_len + 2 * max_read_len + 6 * cigar_stride + (2 * mds_stride + 16) + 192
// (a CIGAR element prints at most 5 digits and its op; an MDS byte of a well-formed stream prints at most 1.5 characters; 192 covers the
// tabs, the integer fields at their widest and the tag names).  A bound that does not fit is NVBIO_ERR_UNSUPPORTED before any launch.
// The MD term holds for well-formed streams only: md_walk reads a byte past the stream as 0, so a stream that mds_stride cuts (or that
// ends) inside a deletion token [3, l, ...] still prints ^, l bases (A for the missing ones) and 0 -- up to 257 characters from two
// bytes, which behind the densest well-formed prefix (1.2 characters a byte) passes 2 * mds_stride + 16 for strides below about 295.
// Nothing unsafe follows: every LDS store is bounded by the class, the length kernel runs the same walk, and such a record is written
// whole where the class has the room and is NVBIO_SAM_STATUS_TOO_LONG where it has not (tests/test_gpu_record_edges.py runs both).  The
// formula stays as it is: widening it would move every caller up a class.
#include "common.h"
#include "record_common.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

static const uint32_t SAM_FIXED_BYTES = 192u;
using SamLdsBytes = Values<1024, 2048, 4096, 8192, 16384>;

enum { SAM_SKIP = 0xFFFFFFFFu };

// the helpers both record formats need -- the bounded LDS writer, cigar_sums, sequence_of, md_walk -- are record_common.h's; here a group is a wave
template <bool EMIT> using SamOut = ByteOut<EMIT, 64u>;

// SEQ and QUAL (output_sam.cpp:365-395), striped: position k of the text is stored symbol (flip ? len - 1 - k : k), complemented when rc
template <bool EMIT>
__device__ __forceinline__ void put_seq_qual(SamOut<EMIT>& o, const nvbio_sam_records& r, const uint32_t r0, const uint32_t rlen, const uint32_t rc)
{
    const bool flip = r.reads_reversed ? !rc : (rc != 0u);
    o.put( '\t' );
    if (EMIT)
    {
        const uint32_t* words = (const uint32_t*)r.reads4_dev;
        for (uint32_t k = o.lane; k < rlen; k += 64u)
        {
            const uint32_t j = r0 + (flip ? rlen - 1u - k : k);
            uint32_t s = (words[j >> 3] >> (28u - 4u * (j & 7u))) & 15u;
            if (rc) s = s < 4u ? 3u - s : 4u;
            o.store( o.at + k, dna_char( s ) );
        }
    }
    o.at += rlen;
    o.put( '\t' );
    if (r.quals_dev == nullptr) { o.put( '*' ); return; }
    if (EMIT)
        for (uint32_t k = o.lane; k < rlen; k += 64u) o.store( o.at + k, (uint8_t)(r.quals_dev[r0 + (flip ? rlen - 1u - k : k)] + 33u) );
    o.at += rlen;
}

// the text of record i, composed by one wave from o.at on; `stage`: mds_stride bytes of the wave's LDS.  Returns its length, SAM_SKIP for a
// record the reference does not write (output_sam.cpp:474-480).
template <bool EMIT>
__device__ uint32_t sam_compose(const nvbio_sam_refs& refs, const nvbio_sam_records& r, const uint32_t i, SamOut<EMIT>& o, uint8_t* stage)
{
    const uint32_t begin = o.at, lane = o.lane;
    const uint32_t st = r.state_dev[i], rc = (st >> 1) & 1u;
    const uint32_t r0 = r.read_index_dev[i], rlen = r.read_index_dev[i + 1u] - r0;
    const uint32_t q0 = r.name_index_dev[i], qlen = r.name_index_dev[i + 1u] - q0;

    uint32_t flags = 4u, pos = 0u, seq = 0u, seq_begin = 0u, ref_len = 0u, clen = 0u;
    const uint16_t* cig = nullptr;
    if (st & 1u)
    {
        clen = r.cigar_lens_dev[i];
        if (clen > r.cigar_stride) return (uint32_t)SAM_SKIP;                  // truncated (0xFFFFFFFF included)
        cig = r.cigars_dev + (size_t)i * r.cigar_stride;
        uint32_t read_sum, text;
        cigar_sums( cig, clen, lane, &read_sum, &ref_len, &text );
        if (read_sum != rlen) return (uint32_t)SAM_SKIP;
        pos = r.pos_dev[i];
        seq = sequence_of( refs, pos );
        seq_begin = refs.sequence_index_dev[seq];
        flags = ((st & 4u) ? 128u : 64u) | (rc ? 16u : 0u);
        if (r.mate_of_dev)
        {
            const uint32_t ms = r.state_dev[r.mate_of_dev[i]];
            flags |= 1u | ((ms & 8u) ? 2u : 0u) | ((ms & 1u) ? 0u : 8u) | ((ms & 2u) ? 32u : 0u);
        }
        if (pos + ref_len > refs.sequence_index_dev[seq + 1u]) flags |= 4u;     // bridges two reference sequences (:459-466)
    }

    o.put_bytes( r.names_dev + q0, qlen );
    o.put( '\t' ); o.put_uint( flags );
    if (flags & 4u)
    {
        o.put_str( "\t*\t0\t0\t*\t*\t0\t0" );
        put_seq_qual( o, r, r0, rlen, rc );
        o.put( '\n' );
        return o.at - begin;
    }

    const uint32_t own_pos = pos - seq_begin + 1u;
    o.put( '\t' ); o.put_bytes( refs.names_dev + refs.names_index_dev[seq], refs.names_index_dev[seq + 1u] - refs.names_index_dev[seq] );
    o.put( '\t' ); o.put_uint( own_pos );
    o.put( '\t' ); o.put_uint( r.mapq_dev[i] );
    o.put( '\t' );
    for (uint32_t c0 = 0u; c0 < clen; c0 += 64u)                               // elements from last to first, each lane one
    {
        const uint32_t e = c0 + lane;
        const uint32_t el = e < clen ? cig[clen - 1u - e] : 0u;
        const uint32_t d = digits_of( el >> 2 ), w = e < clen ? d + 1u : 0u;
        uint32_t end = w;
        for (int s = 1; s < 64; s <<= 1) { const uint32_t t = __shfl_up( end, s, 64 ); if (lane >= (uint32_t)s) end += t; }
        if (EMIT && w) { const uint32_t p = o.at + end - w; o.digits_at( p, el >> 2, d ); o.store( p + d, (uint8_t)"MIDS"[el & 3u] ); }
        o.at += __shfl( end, 63, 64 );
    }

    // RNEXT, PNEXT, TLEN (:482-524)
    o.put( '\t' );
    if (r.mate_of_dev == nullptr) o.put_str( "*\t0\t0" );
    else
    {
        const uint32_t m = r.mate_of_dev[i];
        if (r.state_dev[m] & 1u)
        {
            const uint32_t mpos = r.pos_dev[m], mseq = sequence_of( refs, mpos ), mclen = r.cigar_lens_dev[m];
            uint32_t mread, mref, mtext;
            cigar_sums( r.cigars_dev + (size_t)m * r.cigar_stride, mclen <= r.cigar_stride ? mclen : 0u, lane, &mread, &mref, &mtext );
            int32_t tlen = 0;
            if (mseq == seq)
            {
                o.put( '=' );
                const uint32_t hi = mpos + mref > pos + ref_len ? mpos + mref : pos + ref_len, lo = mpos < pos ? mpos : pos;
                tlen = (int32_t)(hi - lo);
                if (mpos < pos) tlen = -tlen;
            }
            else o.put_bytes( refs.names_dev + refs.names_index_dev[mseq], refs.names_index_dev[mseq + 1u] - refs.names_index_dev[mseq] );
            o.put( '\t' ); o.put_uint( mpos - refs.sequence_index_dev[mseq] + 1u );
            o.put( '\t' ); o.put_int( tlen );
        }
        else { o.put_str( "=\t" ); o.put_uint( own_pos ); o.put_str( "\t0" ); }
    }

    put_seq_qual( o, r, r0, rlen, rc );

    // the tags (:328-339); the counts come from a first walk over the MDS stream, the MD text from a second
    o.put_str( "\tNM:i:" ); o.put_uint( r.ed_dev[i] );
    o.put_str( "\tAS:i:" ); o.put_int( r.score_dev[i] );
    if (r.second_score_dev && r.second_score_dev[i] != NVBIO_SCORE_MIN) { o.put_str( "\tXS:i:" ); o.put_int( r.second_score_dev[i] ); }
    uint32_t mn = 0u;
    if (r.mds_dev)
    {
        mn = r.mds_lens_dev[i] < r.mds_stride ? r.mds_lens_dev[i] : r.mds_stride;
        wave_sync();                                                           // the stage may still be read as the previous use's
        for (uint32_t k = lane; k < mn; k += 64u) stage[k] = r.mds_dev[(size_t)i * r.mds_stride + k];
        wave_sync();
    }
    int32_t mm, gapo, gape;
    SamOut<false> count = { nullptr, 0u, 0u, lane };
    md_walk( stage, mn, count, &mm, &gapo, &gape );
    o.put_str( "\tXM:i:" ); o.put_int( mm );
    o.put_str( "\tXO:i:" ); o.put_int( gapo );
    o.put_str( "\tXG:i:" ); o.put_int( gape );
    o.put_str( "\tMD:Z:" );
    if (count.at == 0u) o.put( '*' ); else md_walk( stage, mn, o, &mm, &gapo, &gape );
    o.put( '\n' );
    return o.at - begin;
}

// ---- step 1: lens[i] = the bytes of record i (0 for a record that is skipped), lens[n] = 0 ----
template <int LDS>
__global__ void __launch_bounds__(256)
sam_lengths_kernel(const nvbio_sam_refs refs, const nvbio_sam_records r, const uint32_t stage_bytes, uint64_t* __restrict__ lens)
{
    __shared__ uint4 lds[4][LDS / 16];
    const uint32_t wave = __builtin_amdgcn_readfirstlane( threadIdx.x >> 6 ), lane = threadIdx.x & 63u;
    const uint64_t i64 = (uint64_t)blockIdx.x * 4u + wave;
    if (i64 > r.n) return;
    if (i64 == r.n) { if (lane == 0u) lens[r.n] = 0ull; return; }
    SamOut<false> o = { nullptr, 0u, 0u, lane };
    const uint32_t len = sam_compose( refs, r, (uint32_t)i64, o, (uint8_t*)lds[wave] + (LDS - stage_bytes) );
    if (lane == 0u) lens[i64] = len == (uint32_t)SAM_SKIP ? 0ull : (uint64_t)len;
}

// ---- step 3: the text of record i at text[offsets[i], offsets[i + 1]) ----
template <int LDS>
__global__ void __launch_bounds__(256)
sam_write_kernel(const nvbio_sam_refs refs, const nvbio_sam_records r, const uint32_t stage_bytes, const uint64_t* __restrict__ offsets,
                 uint8_t* __restrict__ text, const uint64_t capacity, uint32_t* __restrict__ n_skipped, uint32_t* __restrict__ status)
{
    __shared__ uint4 lds[4][LDS / 16];
    const uint32_t wave = __builtin_amdgcn_readfirstlane( threadIdx.x >> 6 ), lane = threadIdx.x & 63u;
    const uint64_t i64 = (uint64_t)blockIdx.x * 4u + wave;
    if (i64 >= r.n) return;
    const uint64_t off = offsets[i64], end = offsets[i64 + 1u];
    uint8_t* buf = (uint8_t*)lds[wave];
    const uint32_t base = (uint32_t)(off & 15u), cap = (uint32_t)LDS - stage_bytes;
    SamOut<true> o = { buf, cap, base, lane };
    const uint32_t len = sam_compose( refs, r, (uint32_t)i64, o, buf + cap );
    uint32_t bad = 0u;
    if (len == (uint32_t)SAM_SKIP) { if (end != off) bad = NVBIO_SAM_STATUS_OFFSETS; else if (lane == 0u) atomicAdd( n_skipped, 1u ); if (!bad) return; }
    else if (end < off || end - off != len) bad = NVBIO_SAM_STATUS_OFFSETS;    // not the offsets of these records
    else if (base + len > cap)              bad = NVBIO_SAM_STATUS_TOO_LONG;    // longer than the declared maxima allow: it was not composed whole
    else if (end > capacity)                bad = NVBIO_SAM_STATUS_CAPACITY;
    if (bad) { if (lane == 0u) atomicOr( status, bad ); return; }
    wave_sync();

    // LDS -> global: the text starts at the residue its offset has, so the body moves as aligned 16-byte words
    uint8_t* dst = text + off;
    const uint32_t head = ((16u - base) & 15u) < len ? ((16u - base) & 15u) : len;
    if (lane < head) dst[lane] = buf[base + lane];
    const uint32_t body = (len - head) >> 4, tail = len - head - (body << 4);
    const uint4* src16 = (const uint4*)(buf + base + head);
    uint4*       dst16 = (uint4*)(dst + head);
    for (uint32_t k = lane; k < body; k += 64u) dst16[k] = src16[k];
    if (lane < tail) dst[head + (body << 4) + lane] = buf[base + head + (body << 4) + lane];
}

struct SamPlan { uint32_t lds, stage; };

// the checks of both calls that need no device, and the LDS a wave needs
static nvbio_status sam_plan(const nvbio_sam_refs* refs, const nvbio_sam_records* r, uint32_t flags, uint32_t known_flags, SamPlan* plan)
{
    NVB_REQUIRE( refs != nullptr && r != nullptr, "refs or records is NULL" );
    NVB_REQUIRE( (flags & ~known_flags) == 0u, "unknown flags" );
    NVB_REQUIRE( r->n < 0x7FFFFFFFu, "n too large" );
    plan->lds = 1024u; plan->stage = 0u;
    if (r->n == 0u) return NVBIO_OK;
    NVB_REQUIRE( refs->n_seqs > 0u && refs->sequence_index_dev && refs->names_dev && refs->names_index_dev, "refs: NULL device pointer or no sequence" );
    NVB_REQUIRE( r->names_dev && r->name_index_dev && r->reads4_dev && r->read_index_dev && r->state_dev && r->pos_dev && r->score_dev && r->ed_dev &&
                 r->mapq_dev && r->cigars_dev && r->cigar_lens_dev, "records: NULL device pointer" );
    NVB_REQUIRE( r->mds_dev == nullptr || (r->mds_lens_dev != nullptr && r->mds_stride >= 2u), "mds_dev needs mds_lens_dev and mds_stride >= 2" );
    NVB_REQUIRE( r->max_read_len < 1024u, "max_read_len must be below 1024" );
    const uint64_t stage = r->mds_dev ? ((uint64_t)r->mds_stride + 15u) & ~15ull : 0u;
    const uint64_t md    = r->mds_dev ? 2ull * r->mds_stride + 16u : 1u;
    const uint64_t bound = (uint64_t)r->max_name_len + 2ull * refs->max_name_len + 2ull * r->max_read_len + 6ull * r->cigar_stride + md + SAM_FIXED_BYTES;
    const uint64_t need  = 16u + bound + stage;
    uint32_t lds = 0u;
    for (const uint32_t c : { 1024u, 2048u, 4096u, 8192u, 16384u }) if (!lds && need <= c) lds = c;
    if (!lds)
    {
        set_error( "sam: a record may take %llu bytes (names %u + 2 x %u, reads %u, cigar_stride %u, mds_stride %u) and a wave's LDS holds 16384 with %llu "
                   "taken by the MDS stage and the alignment residue", (unsigned long long)bound, r->max_name_len, refs->max_name_len, r->max_read_len,
                   r->cigar_stride, r->mds_dev ? r->mds_stride : 0u, (unsigned long long)(stage + 16u) );
        return NVBIO_ERR_UNSUPPORTED;
    }
    plan->lds = lds; plan->stage = (uint32_t)stage;
    return NVBIO_OK;
}

static nvbio_status sam_scan_bytes(uint32_t n, size_t* bytes)
{
    NVB_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, *bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n + 1u), (hipStream_t)0 ) );
    return NVBIO_OK;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_sam_format_temp_bytes(uint32_t n, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    NVB_REQUIRE( n < 0x7FFFFFFFu, "n too large" );
    size_t work = 0; NVB_CHECK( sam_scan_bytes( n, &work ) );
    *bytes = ScratchLayout::round( work ) + 256u;
    return NVBIO_OK;
}

nvbio_status nvbio_sam_record_offsets(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, uint64_t* offsets_dev,
                                      void* temp_dev, uint64_t temp_bytes, void* stream)
{
    SamPlan plan; NVB_CHECK( sam_plan( refs, records, flags, NVBIO_SAM_LENGTHS_ONLY, &plan ) );
    NVB_REQUIRE( offsets_dev != nullptr, "offsets_dev is NULL" );
    const uint32_t n = records->n;
    NVB_REQUIRE( n == 0u || temp_dev != nullptr, "temp_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0u) { NVB_HIP( hipMemsetAsync( offsets_dev, 0, sizeof(uint64_t), s ) ); return NVBIO_OK; }
    size_t work = 0; NVB_CHECK( sam_scan_bytes( n, &work ) );                 // rocPRIM sizes its temp for the current device
    const uint64_t skip = (256u - ((uintptr_t)temp_dev & 255u)) & 255u;
    NVB_REQUIRE( temp_bytes >= skip + work, "temp_bytes too small (nvbio_sam_format_temp_bytes)" );
    const dim3 grid( (unsigned)(((uint64_t)n + 1u + 3u) / 4u) );
    NVB_CHECK( with_value( SamLdsBytes(), (int)plan.lds, [&](auto L) {
        return NVB_LAUNCH( (sam_lengths_kernel<decltype(L)::value>), grid, dim3(256), s, *refs, *records, plan.stage, offsets_dev );
    }, []() { set_error( "sam: no kernel for this LDS size" ); return NVBIO_ERR_UNSUPPORTED; } ) );
    if (flags & NVBIO_SAM_LENGTHS_ONLY) return NVBIO_OK;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum( (uint8_t*)temp_dev + skip, work, offsets_dev, offsets_dev, (int)(n + 1u), s );
    if (e != hipSuccess) { set_error( "sam_record_offsets: scan failed: %s", hipGetErrorString( e ) ); return NVBIO_ERR_HIP; }
    return NVBIO_OK;
}

nvbio_status nvbio_sam_format(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, const uint64_t* offsets_dev,
                              uint8_t* text_dev, uint64_t text_capacity, uint32_t* n_skipped_dev, uint32_t* status_dev, void* stream)
{
    SamPlan plan; NVB_CHECK( sam_plan( refs, records, flags, 0u, &plan ) );
    NVB_REQUIRE( n_skipped_dev != nullptr && status_dev != nullptr, "n_skipped_dev or status_dev is NULL" );
    const uint32_t n = records->n;
    NVB_REQUIRE( n == 0u || offsets_dev != nullptr, "offsets_dev is NULL" );
    NVB_REQUIRE( n == 0u || text_capacity == 0u || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)text_dev & 15u) == 0u, "text_dev must be 16-byte aligned" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    NVB_HIP( hipMemsetAsync( n_skipped_dev, 0, sizeof(uint32_t), s ) );
    if (n == 0u) return NVBIO_OK;
    const dim3 grid( (unsigned)(((uint64_t)n + 3u) / 4u) );
    return with_value( SamLdsBytes(), (int)plan.lds, [&](auto L) {
        return NVB_LAUNCH( (sam_write_kernel<decltype(L)::value>), grid, dim3(256), s, *refs, *records, plan.stage, offsets_dev, text_dev, text_capacity,
                           n_skipped_dev, status_dev );
    }, []() { set_error( "sam: no kernel for this LDS size" ); return NVBIO_ERR_UNSUPPORTED; } );
}

} // extern "C"
