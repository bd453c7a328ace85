// bam.hip -- nvBowtie's BAM records and the BGZF container around them, made on the device (gfx950):
//         generate_cigar, generate_md_string, encode_bp             nvbio/io/output/output_bam.cpp:65-93,140-213,216-225
//         process_one_alignment, output_alignment                   nvbio/io/output/output_bam.cpp:227-471,495-544
//         GzipCompressor / BGZFCompressor (the framing only)        nvbio/io/output/output_gzip.cpp:29-42,118-134
// The records are a pure function of the arrays sam.hip prints from, and are made in the same three steps: the byte length of every
// record, an exclusive uint64 scan (three small launches here, whose temp is a host formula: 8 bytes per 2048 records), the write.
//
// Shape of the two record kernels: ONE RECORD PER GROUP OF 16 LANES, four records to a wave, 16 to a 256-lane workgroup (DESIGN 4.12
// found the SAM kernel's time in per-record scalar work that occupies a whole wave; a BAM record has far less of it and four records now
// share its issue slots).  A group's control flow is uniform -- its record index is the same in its 16 lanes -- and its lanes stripe
// the name, the CIGAR elements, QUAL, and SEQ, where a lane takes 8 symbols at a time: one or two 32-bit words of the 4-bit read, turned
// and complemented as a word, give 4 bytes of SEQ.  The write kernel composes the record in LDS at the byte residue (mod 16) its global
// offset has and copies it out: byte stores for the unaligned head and tail only, 16-byte stores from 16-byte LDS reads for the body.
// The length kernel runs the same code with the stores compiled out (ByteOut<EMIT, 16>), so the two cannot disagree; the write kernel
// still compares its own length with the caller's offsets and refuses a record that differs.
//
// Limit: a group's LDS holds BAM_LDS[k] bytes (at most 16384; a workgroup is kept to 64 KiB of static LDS -- a choice, the limit of the
// CDNA parts before gfx950, which accepts more -- so groups of 8192 / 16384 bytes come 8 / 4 to a workgroup), of which 16 go to the residue and mds_stride (rounded up to 16) to the staged MDS stream.  The bound on a record:
//   max_name_len + 4 * cigar_stride + max_read_len + (max_read_len + 1) / 2 + (2 * mds_stride + 16) + 72
// A bound that does not fit is NVBIO_ERR_UNSUPPORTED before any launch.  The MD term (1.5 characters an MDS byte) holds for well-formed
// streams; a stream cut inside a deletion token can print more (sam.hip says how), and then the record is whole where the class has
// the room and NVBIO_BAM_STATUS_TOO_LONG where it has not: the stores are bounded either way.
//
// The BGZF kernel: one workgroup per block of 65280 payload bytes.  A lane loads 16-byte words of the (aligned) payload, a row of 256
// words at a time; the payload lands at byte 23 of its block, so the destination's 16-byte words are cut from two source words each
// with a byte shift that is uniform over the block.  The CRC-32 rides on the same registers: a lane folds its words into one raw
// remainder (slicing-by-4 for the word, a byte-sliced table for the multiplication by x^(8 * 4096) that carries the remainder from one
// row to the next), multiplies it by x^(8 * the bytes behind its last word) -- a product of the host's x^(8 * 2^k) mod P -- and the
// workgroup XORs the 256 results: crc( A || B ) = crc( A ) x^(8 |B|) + crc( B ) over raw remainders.  The initial complement enters as
// 0xFFFFFFFF x^(8 L) and the final one is applied once.  No atomics.
#include "common.h"
#include "record_common.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

static const uint32_t BAM_FIXED_BYTES = 72u;
static const uint32_t BAM_GROUP = 16u;                                          // lanes to a record
using BamLdsBytes = Values<512, 1024, 2048, 4096, 8192, 16384>;
template <int LDS> struct BamGroups { static constexpr int value = LDS <= 4096 ? 16 : 65536 / LDS; };    // records to a workgroup

enum { BAM_SKIP = 0xFFFFFFFFu };

template <bool EMIT>
struct BamOut : ByteOut<EMIT, BAM_GROUP>
{
    __device__ __forceinline__ void put_u32(const uint32_t v) { for (uint32_t k = 0; k < 4u; ++k) this->put( (uint8_t)(v >> (8u * k)) ); }
    __device__ __forceinline__ void put_tag_c(const char a, const char b, const uint32_t v) { this->put( a ); this->put( b ); this->put( 'c' ); this->put( (uint8_t)v ); }
    __device__ __forceinline__ void put_tag_i(const char a, const char b, const uint32_t v) { this->put( a ); this->put( b ); this->put( 'i' ); put_u32( v ); }
};

// the SAM specification's reg2bin (section 5.3) of the 0-based half-open interval [beg, end)
__device__ __forceinline__ uint32_t reg2bin(const int32_t beg, int32_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}

// 8 symbols of a 4-bit word (symbol q in bits [28 - 4 q, 31 - 4 q]) -> their BAM codes in the same places: complemented when rc (s < 4 ->
// 3 - s), then s < 4 -> 1 << s, any other -> 15 (encode_bp); the symbols from `cnt` on give 0
__device__ __forceinline__ uint32_t bam_codes(const uint32_t x, const uint32_t cnt, const uint32_t rc)
{
    uint32_t out = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q)
    {
        uint32_t s = (x >> (28u - 4u * q)) & 15u;
        if (rc && s < 4u) s = 3u - s;
        const uint32_t code = s < 4u ? 1u << s : 15u;
        if (q < cnt) out |= code << (28u - 4u * q);
    }
    return out;
}

// SEQ and QUAL (output_bam.cpp:254-306): position k of either is stored symbol (flip ? len - 1 - k : k).  A lane takes the 8 positions
// [8 c, 8 c + 8) of SEQ: they are 8 stored symbols in a row, in one or two words of the read, in order or turned round.
template <bool EMIT>
__device__ __forceinline__ void put_seq_qual(BamOut<EMIT>& o, const nvbio_sam_records& r, const uint32_t r0, const uint32_t rlen, const uint32_t rc)
{
    const bool flip = r.reads_reversed ? !rc : (rc != 0u);
    if (EMIT)
    {
        const uint32_t* words = (const uint32_t*)r.reads4_dev;
        for (uint32_t k0 = 8u * o.lane; k0 < rlen; k0 += 8u * BAM_GROUP)
        {
            const uint32_t cnt = rlen - k0 < 8u ? rlen - k0 : 8u;
            const uint32_t jl  = r0 + (flip ? rlen - k0 - cnt : k0), sh = jl & 7u;       // the first of the cnt stored symbols
            const uint32_t w0  = words[jl >> 3], w1 = sh + cnt > 8u ? words[(jl >> 3) + 1u] : 0u;
            uint32_t x = (uint32_t)(((((uint64_t)w0 << 32) | w1) << (4u * sh)) >> 32);   // symbol jl + q in nibble q from the top, q < cnt
            if (flip)
            {
                x = __builtin_bswap32( x );
                x = ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu);                 // nibble q <- nibble 7 - q ...
                x <<= 4u * (8u - cnt) & 31u;                                             // ... <- nibble cnt - 1 - q (cnt >= 1)
            }
            const uint32_t codes = bam_codes( x, cnt, rc );
            for (uint32_t b = 0; b < (cnt + 1u) >> 1; ++b) o.store( o.at + (k0 >> 1) + b, (uint8_t)(codes >> (24u - 8u * b)) );
        }
    }
    o.at += (rlen + 1u) >> 1;
    if (EMIT)
        for (uint32_t k = o.lane; k < rlen; k += BAM_GROUP)
            o.store( o.at + k, r.quals_dev ? r.quals_dev[r0 + (flip ? rlen - 1u - k : k)] : (uint8_t)0xFFu );
    o.at += rlen;
}

// the bytes of record i, composed by one group from o.at on; `stage`: mds_stride bytes of the group's LDS.  Returns its length, BAM_SKIP
// for a record the reference does not write (output_bam.cpp:399-405).
template <bool EMIT>
__device__ uint32_t bam_compose(const nvbio_sam_refs& refs, const nvbio_sam_records& r, const uint32_t i, const uint32_t call_flags, BamOut<EMIT>& o,
                                uint8_t* stage)
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
        if (clen > r.cigar_stride) return (uint32_t)BAM_SKIP;                  // truncated (0xFFFFFFFF included)
        cig = r.cigars_dev + (size_t)i * r.cigar_stride;
        uint32_t read_sum, text;
        cigar_sums<BAM_GROUP>( cig, clen, lane, &read_sum, &ref_len, &text );
        if (read_sum != rlen) return (uint32_t)BAM_SKIP;
        pos = r.pos_dev[i];
        seq = sequence_of( refs, pos );
        seq_begin = refs.sequence_index_dev[seq];
        flags = ((st & 4u) ? 128u : 64u) | (rc ? 16u : 0u);                    // :346-368
        if (r.mate_of_dev)
        {
            const uint32_t ms = r.state_dev[r.mate_of_dev[i]];
            flags |= 1u | ((ms & 8u) ? 2u : 0u) | ((ms & 1u) ? 0u : 8u) | ((ms & 2u) ? 32u : 0u);
        }
        if (pos + ref_len > refs.sequence_index_dev[seq + 1u]) flags |= 4u;     // bridges two reference sequences (:370-385)
    }

    // the eight fixed words behind block_size (:501-508); a record written as unmapped keeps the -1s and carries neither MAPQ nor CIGAR
    const bool mapped = (flags & 4u) == 0u;
    int32_t  ref_id = -1, own_pos = -1, next_ref = -1, next_pos = -1, tlen = 0;
    uint32_t bin = (call_flags & NVBIO_BAM_REG2BIN) ? 4680u : 0u, mapq = 0u;
    if (mapped)
    {
        ref_id = (int32_t)seq; own_pos = (int32_t)(pos - seq_begin); mapq = r.mapq_dev[i];
        if (call_flags & NVBIO_BAM_REG2BIN) bin = reg2bin( own_pos, (int32_t)((uint32_t)own_pos + ref_len) );
        if (r.mate_of_dev)                                                     // :407-451
        {
            const uint32_t m = r.mate_of_dev[i];
            if (r.state_dev[m] & 1u)
            {
                const uint32_t mpos = r.pos_dev[m], mseq = sequence_of( refs, mpos ), mclen = r.cigar_lens_dev[m];
                uint32_t mread, mref, mtext;
                cigar_sums<BAM_GROUP>( r.cigars_dev + (size_t)m * r.cigar_stride, mclen <= r.cigar_stride ? mclen : 0u, lane, &mread, &mref, &mtext );
                next_ref = (int32_t)mseq; next_pos = (int32_t)(mpos - refs.sequence_index_dev[mseq]);
                if (mseq == seq)
                {
                    const uint32_t hi = mpos + mref > pos + ref_len ? mpos + mref : pos + ref_len, lo = mpos < pos ? mpos : pos;
                    tlen = (int32_t)(hi - lo);
                    if (mpos < pos) tlen = -tlen;
                }
            }
            else { next_ref = ref_id; next_pos = own_pos; }
        }
    }
    const uint32_t n_cigar = mapped ? clen : 0u;
    if (EMIT && lane >= 1u && lane <= 8u)
    {
        const uint32_t w = lane == 1u ? (uint32_t)ref_id : lane == 2u ? (uint32_t)own_pos : lane == 3u ? (bin << 16 | mapq << 8 | (qlen + 1u)) :
                           lane == 4u ? (flags << 16 | n_cigar) : lane == 5u ? rlen : lane == 6u ? (uint32_t)next_ref : lane == 7u ? (uint32_t)next_pos :
                           (uint32_t)tlen;
        for (uint32_t k = 0; k < 4u; ++k) o.store( o.at + 4u * lane + k, (uint8_t)(w >> (8u * k)) );
    }
    o.at += 36u;

    o.put_bytes( r.names_dev + q0, qlen );
    o.put( 0u );
    if (EMIT)                                                                  // elements from last to first (:65-93)
        for (uint32_t e = lane; e < n_cigar; e += BAM_GROUP)
        {
            const uint32_t el = cig[clen - 1u - e], t = el & 3u, w = (el >> 2) << 4 | (t == 3u ? 4u : t);
            for (uint32_t k = 0; k < 4u; ++k) o.store( o.at + 4u * e + k, (uint8_t)(w >> (8u * k)) );
        }
    o.at += 4u * n_cigar;
    put_seq_qual( o, r, r0, rlen, rc );

    if (mapped)                                                                // the tags (:520-534)
    {
        o.put_tag_c( 'N', 'M', r.ed_dev[i] );
        o.put_tag_i( 'A', 'S', (uint32_t)r.score_dev[i] );
        if (r.second_score_dev && r.second_score_dev[i] != NVBIO_SCORE_MIN) o.put_tag_i( 'X', 'S', (uint32_t)r.second_score_dev[i] );
        uint32_t mn = 0u;
        if (r.mds_dev)
        {
            mn = r.mds_lens_dev[i] < r.mds_stride ? r.mds_lens_dev[i] : r.mds_stride;
            for (uint32_t k = lane; k < mn; k += BAM_GROUP) stage[k] = r.mds_dev[(size_t)i * r.mds_stride + k];
            wave_sync();
        }
        // one walk: the MD text goes where it belongs, behind XM XO XG (12 bytes) and its own tag's 3; the counts it gives are stored after
        const uint32_t tags_at = o.at;
        o.at += 15u;
        int32_t mm, gapo, gape;
        md_walk( stage, mn, o, &mm, &gapo, &gape );
        const bool has_md = o.at != tags_at + 15u;
        if (has_md) o.put( 0u );
        const uint32_t end = has_md ? o.at : tags_at + 12u;
        o.at = tags_at;
        o.put_tag_c( 'X', 'M', (uint32_t)mm ); o.put_tag_c( 'X', 'O', (uint32_t)gapo ); o.put_tag_c( 'X', 'G', (uint32_t)gape );
        if (has_md) { o.put( 'M' ); o.put( 'D' ); o.put( 'Z' ); }
        o.at = end;
    }
    const uint32_t len = o.at - begin;
    if (EMIT && lane < 4u) o.store( begin + lane, (uint8_t)((len - 4u) >> (8u * lane)) );
    return len;
}

// ---- step 1: lens[i] = the bytes of record i (0 for a record that is skipped), lens[n] = 0 ----
template <int LDS>
__global__ void __launch_bounds__(16 * BamGroups<LDS>::value)
bam_lengths_kernel(const nvbio_sam_refs refs, const nvbio_sam_records r, const uint32_t flags, const uint32_t stage_bytes, uint64_t* __restrict__ lens)
{
    constexpr uint32_t G = BamGroups<LDS>::value;
    __shared__ uint4 lds[G][LDS / 16];
    const uint32_t group = threadIdx.x / BAM_GROUP, lane = threadIdx.x % BAM_GROUP;
    const uint64_t i64 = (uint64_t)blockIdx.x * G + group;
    if (i64 > r.n) return;
    if (i64 == r.n) { if (lane == 0u) lens[r.n] = 0ull; return; }
    BamOut<false> o; o.buf = nullptr; o.cap = 0u; o.at = 0u; o.lane = lane;
    const uint32_t len = bam_compose( refs, r, (uint32_t)i64, flags, o, (uint8_t*)lds[group] + (LDS - stage_bytes) );
    if (lane == 0u) lens[i64] = len == (uint32_t)BAM_SKIP ? 0ull : (uint64_t)len;
}

// ---- step 3: the bytes of record i at data[offsets[i], offsets[i + 1]) ----
template <int LDS>
__global__ void __launch_bounds__(16 * BamGroups<LDS>::value)
bam_write_kernel(const nvbio_sam_refs refs, const nvbio_sam_records r, const uint32_t flags, const uint32_t stage_bytes, const uint64_t* __restrict__ offsets,
                 uint8_t* __restrict__ data, const uint64_t capacity, uint32_t* __restrict__ n_skipped, uint32_t* __restrict__ status)
{
    constexpr uint32_t G = BamGroups<LDS>::value;
    __shared__ uint4 lds[G][LDS / 16];
    const uint32_t group = threadIdx.x / BAM_GROUP, lane = threadIdx.x % BAM_GROUP;
    const uint64_t i64 = (uint64_t)blockIdx.x * G + group;
    if (i64 >= r.n) return;
    const uint64_t off = offsets[i64], end = offsets[i64 + 1u];
    uint8_t* buf = (uint8_t*)lds[group];
    const uint32_t base = (uint32_t)(off & 15u), cap = (uint32_t)LDS - stage_bytes;
    BamOut<true> o; o.buf = buf; o.cap = cap; o.at = base; o.lane = lane;
    const uint32_t len = bam_compose( refs, r, (uint32_t)i64, flags, o, buf + cap );
    uint32_t bad = 0u;
    if (len == (uint32_t)BAM_SKIP) { if (end != off) bad = NVBIO_BAM_STATUS_OFFSETS; else if (lane == 0u) atomicAdd( n_skipped, 1u ); if (!bad) return; }
    else if (end < off || end - off != len) bad = NVBIO_BAM_STATUS_OFFSETS;    // not the offsets of these records
    else if (base + len > cap)              bad = NVBIO_BAM_STATUS_TOO_LONG;    // longer than the declared maxima allow: it was not composed whole
    else if (end > capacity)                bad = NVBIO_BAM_STATUS_CAPACITY;
    if (bad) { if (lane == 0u) atomicOr( status, bad ); return; }
    wave_sync();

    // LDS -> global: the record starts at the residue its offset has, so the body moves as aligned 16-byte words
    uint8_t* dst = data + off;
    const uint32_t head = ((16u - base) & 15u) < len ? ((16u - base) & 15u) : len;
    if (lane < head) dst[lane] = buf[base + lane];
    const uint32_t body = (len - head) >> 4, tail = len - head - (body << 4);
    const uint4* src16 = (const uint4*)(buf + base + head);
    uint4*       dst16 = (uint4*)(dst + head);
    for (uint32_t k = lane; k < body; k += BAM_GROUP) dst16[k] = src16[k];
    if (lane < tail) dst[head + (body << 4) + lane] = buf[base + head + (body << 4) + lane];
}

struct BamPlan { uint32_t lds, stage; };

// the checks of both calls that need no device, and the LDS a group needs
static nvbio_status bam_plan(const nvbio_sam_refs* refs, const nvbio_sam_records* r, uint32_t flags, uint32_t known_flags, BamPlan* plan)
{
    NVB_REQUIRE( refs != nullptr && r != nullptr, "refs or records is NULL" );
    NVB_REQUIRE( (flags & ~known_flags) == 0u, "unknown flags" );
    NVB_REQUIRE( r->n < 0x7FFFFFFFu, "n too large" );
    plan->lds = 512u; plan->stage = 0u;
    if (r->n == 0u) return NVBIO_OK;
    NVB_REQUIRE( refs->n_seqs > 0u && refs->sequence_index_dev && refs->names_dev && refs->names_index_dev, "refs: NULL device pointer or no sequence" );
    NVB_REQUIRE( r->names_dev && r->name_index_dev && r->reads4_dev && r->read_index_dev && r->state_dev && r->pos_dev && r->score_dev && r->ed_dev &&
                 r->mapq_dev && r->cigars_dev && r->cigar_lens_dev, "records: NULL device pointer" );
    NVB_REQUIRE( r->mds_dev == nullptr || (r->mds_lens_dev != nullptr && r->mds_stride >= 2u), "mds_dev needs mds_lens_dev and mds_stride >= 2" );
    NVB_REQUIRE( r->max_read_len < 1024u, "max_read_len must be below 1024" );
    if (r->max_name_len > 254u) { set_error( "bam: max_name_len %u: l_read_name is one byte and counts the NUL, so a name has at most 254", r->max_name_len ); return NVBIO_ERR_UNSUPPORTED; }
    if (r->cigar_stride > 65535u) { set_error( "bam: cigar_stride %u: n_cigar_op has 16 bits", r->cigar_stride ); return NVBIO_ERR_UNSUPPORTED; }
    const uint64_t stage = r->mds_dev ? ((uint64_t)r->mds_stride + 15u) & ~15ull : 0u;
    const uint64_t md    = r->mds_dev ? 2ull * r->mds_stride + 16u : 0u;
    const uint64_t bound = (uint64_t)r->max_name_len + 4ull * r->cigar_stride + r->max_read_len + (r->max_read_len + 1u) / 2u + md + BAM_FIXED_BYTES;
    const uint64_t need  = 16u + bound + stage;
    uint32_t lds = 0u;
    for (const uint32_t c : { 512u, 1024u, 2048u, 4096u, 8192u, 16384u }) if (!lds && need <= c) lds = c;
    if (!lds)
    {
        set_error( "bam: a record may take %llu bytes (name %u, reads %u, cigar_stride %u, mds_stride %u) and a group's LDS holds 16384 with %llu taken by "
                   "the MDS stage and the alignment residue", (unsigned long long)bound, r->max_name_len, r->max_read_len, r->cigar_stride,
                   r->mds_dev ? r->mds_stride : 0u, (unsigned long long)(stage + 16u) );
        return NVBIO_ERR_UNSUPPORTED;
    }
    plan->lds = lds; plan->stage = (uint32_t)stage;
    return NVBIO_OK;
}

// ---- step 2: the exclusive uint64 scan of lens[0, n + 1), in place.  Three launches over tiles of 2048 values, so that the temp is 8 bytes a
// tile whatever the device: the tiles' sums, their scan by one workgroup, and each tile's own scan from its sum's prefix ----
static const uint32_t SCAN_TILE = 2048u;                                        // 256 lanes x 8 values

__global__ void __launch_bounds__(256)
bam_tile_sums_kernel(const uint64_t* __restrict__ v, const uint32_t count, uint64_t* __restrict__ sums)
{
    using Reduce = hipcub::BlockReduce<uint64_t, 256>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 8u;
    uint64_t s = 0ull;
    for (uint32_t k = 0; k < 8u; ++k) if (base + k < count) s += v[base + k];
    s = Reduce( tmp ).Sum( s );
    if (threadIdx.x == 0u) sums[blockIdx.x] = s;
}

__global__ void __launch_bounds__(1024)
bam_scan_sums_kernel(uint64_t* __restrict__ sums, const uint32_t tiles)
{
    using Scan = hipcub::BlockScan<uint64_t, 1024>;
    __shared__ typename Scan::TempStorage tmp;
    uint64_t carry = 0ull;
    for (uint32_t base = 0; base < tiles; base += 1024u)
    {
        const uint32_t j = base + threadIdx.x;
        uint64_t x = j < tiles ? sums[j] : 0ull, total;
        Scan( tmp ).ExclusiveSum( x, x, total );
        if (j < tiles) sums[j] = carry + x;
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
bam_tile_scan_kernel(uint64_t* __restrict__ v, const uint32_t count, const uint64_t* __restrict__ sums)
{
    using Scan = hipcub::BlockScan<uint64_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 8u;
    uint64_t x[8], s = 0ull;
    for (uint32_t k = 0; k < 8u; ++k) { x[k] = base + k < count ? v[base + k] : 0ull; s += x[k]; }
    uint64_t before;
    Scan( tmp ).ExclusiveSum( s, before );
    before += sums[blockIdx.x];
    for (uint32_t k = 0; k < 8u; ++k) { if (base + k < count) v[base + k] = before; before += x[k]; }
}

static uint64_t bam_scan_bytes(uint32_t n) { return 8ull * (((uint64_t)n + 1u + SCAN_TILE - 1u) / SCAN_TILE); }

// ---- BGZF --------------------------------------------------------------------------------------------------------------------------
static const uint32_t CRC_POLY = 0xEDB88320u;                                   // zlib's, reflected: bit 31 is x^0
static const uint32_t BGZF_ROW_LOG2 = 12u;                                      // a row of 256 16-byte words: 2^12 bytes

// a b mod P over GF(2), reflected (zlib's multmodp)
__host__ __device__ inline uint32_t gf2_mul(const uint32_t a, uint32_t b)
{
    uint32_t p = 0u;
    for (uint32_t k = 0; k < 32u; ++k) { if (a & (0x80000000u >> k)) p ^= b; b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u); }
    return p;
}

struct BgzfConsts { uint32_t x2k[16]; };                                        // x^(8 * 2^k) mod P: what k zero... 2^k zero bytes do to a remainder

static const BgzfConsts& bgzf_consts()
{
    static const BgzfConsts c = [] {
        BgzfConsts v;
        uint32_t p = 0x80000000u;                                               // x^0
        for (int k = 0; k < 8; ++k) p = (p >> 1) ^ ((p & 1u) ? CRC_POLY : 0u);  // x^8
        for (int k = 0; k < 16; ++k) { v.x2k[k] = p; p = gf2_mul( p, p ); }
        return v;
    }();
    return c;
}

// x^(8 n) mod P, n < 65536
__device__ __forceinline__ uint32_t x_pow_bytes(const BgzfConsts& K, const uint32_t n)
{
    uint32_t p = 0x80000000u;
    for (uint32_t k = 0; k < 16u; ++k) if ((n >> k) & 1u) p = gf2_mul( p, K.x2k[k] );
    return p;
}

// source word k of a payload of L bytes: whole when it lies inside, else its bytes below L and zeros
__device__ __forceinline__ uint4 bgzf_load_word(const uint8_t* __restrict__ src, const uint32_t k, const uint32_t L)
{
    if (16u * k + 16u <= L) return ((const uint4*)src)[k];
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (uint32_t q = 0; q < 16u; ++q) if (16u * k + q < L) w[q >> 2] |= (uint32_t)src[16u * k + q] << (8u * (q & 3u));
    return make_uint4( w[0], w[1], w[2], w[3] );
}

// bytes [sh, sh + 16) of the 32 bytes A || B, 0 < sh < 16: WSH = sh / 4 words and bsh = sh % 4 bytes
template <uint32_t WSH>
__device__ __forceinline__ uint4 bgzf_cut(const uint4 A, const uint4 B, const uint32_t bsh)
{
    const uint32_t w[8] = { A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w };
    uint32_t o[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) o[j] = (uint32_t)((((uint64_t)w[j + WSH + 1u] << 32) | w[j + WSH]) >> (8u * bsh));
    return make_uint4( o[0], o[1], o[2], o[3] );
}

__global__ void __launch_bounds__(256)
bgzf_frame_kernel(const uint8_t* __restrict__ data, const uint64_t n_bytes, uint8_t* __restrict__ out, const BgzfConsts K)
{
    __shared__ uint32_t T[4][256];                                              // slicing-by-4 tables of the raw CRC: T[j][v] = v x^(8 (j + 1)) ... of byte v
    __shared__ uint32_t S[4][256];                                              // S[j][v] = (v << 8 j) x^(8 * 4096): a remainder carried over one row
    __shared__ uint32_t part[4];
    const uint32_t t = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t L = (uint32_t)(n_bytes - b * NVBIO_BGZF_BLOCK_BYTES < NVBIO_BGZF_BLOCK_BYTES ? n_bytes - b * NVBIO_BGZF_BLOCK_BYTES : NVBIO_BGZF_BLOCK_BYTES);
    const uint8_t* __restrict__ src = data + b * NVBIO_BGZF_BLOCK_BYTES;         // 16-byte aligned: 65280 = 16 * 4080
    uint8_t* __restrict__ blk = out + b * (NVBIO_BGZF_BLOCK_BYTES + NVBIO_BGZF_OVERHEAD);
    uint8_t* __restrict__ dst = blk + 23u;

    {
        uint32_t c = t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        T[0][t] = c;
        for (uint32_t j = 0; j < 4u; ++j) S[j][t] = gf2_mul( t << (8u * j), K.x2k[BGZF_ROW_LOG2] );
        __syncthreads();
        for (uint32_t j = 1; j < 4u; ++j) { c = T[0][c & 255u] ^ (c >> 8); T[j][t] = c; }
        __syncthreads();
    }

    if (t == 0u)                                                                // the 18 + 5 bytes before the payload
    {
        const uint32_t bsize = L + NVBIO_BGZF_OVERHEAD - 1u, nlen = ~L & 0xFFFFu;
        const uint8_t h[23] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8),
                                1, (uint8_t)L, (uint8_t)(L >> 8), (uint8_t)nlen, (uint8_t)(nlen >> 8) };
        for (uint32_t k = 0; k < 23u; ++k) blk[k] = h[k];
    }

    // the destination's first aligned byte is payload byte `head`: destination word m = payload bytes [head + 16 m, head + 16 m + 16)
    const uint32_t res  = (uint32_t)((b * (NVBIO_BGZF_BLOCK_BYTES + NVBIO_BGZF_OVERHEAD) + 23u) & 15u);
    const uint32_t sh   = (16u - res) & 15u, head = sh < L ? sh : L;
    const uint32_t n_src = L >> 4, body = (L - head) >> 4, tail = L - head - (body << 4);      // body <= n_src
    uint4* dst16 = (uint4*)(dst + head);
    if (t < head) dst[t] = src[t];
    if (t < tail) dst[head + (body << 4) + t] = src[head + (body << 4) + t];

    uint32_t acc = 0u, last = 0u, any = 0u;
    for (uint32_t m = t; m < n_src; m += 256u)
    {
        const uint4 A = ((const uint4*)src)[m];
        acc = S[0][acc & 255u] ^ S[1][(acc >> 8) & 255u] ^ S[2][(acc >> 16) & 255u] ^ S[3][acc >> 24];
        uint32_t c = 0u;
        const uint32_t d[4] = { A.x, A.y, A.z, A.w };
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) { c ^= d[j]; c = T[3][c & 255u] ^ T[2][(c >> 8) & 255u] ^ T[1][(c >> 16) & 255u] ^ T[0][c >> 24]; }
        acc ^= c;
        last = m; any = 1u;
        if (m < body)
        {
            uint4 o = A;
            if (sh)
            {
                const uint4 B = bgzf_load_word( src, m + 1u, L );
                const uint32_t bsh = sh & 3u;
                switch (sh >> 2) { case 0: o = bgzf_cut<0>( A, B, bsh ); break; case 1: o = bgzf_cut<1>( A, B, bsh ); break;
                                   case 2: o = bgzf_cut<2>( A, B, bsh ); break; default: o = bgzf_cut<3>( A, B, bsh ); }
            }
            dst16[m] = o;
        }
    }
    // this lane's remainder, moved over the bytes behind its last word; lane 255 adds the initial complement moved over the whole payload,
    // lane 254 the bytes behind the last whole word
    uint32_t v = any ? gf2_mul( acc, x_pow_bytes( K, L - 16u * (last + 1u) ) ) : 0u;
    if (t == 255u) v ^= gf2_mul( 0xFFFFFFFFu, x_pow_bytes( K, L ) );
    if (t == 254u)
    {
        uint32_t c = 0u;
        for (uint32_t k = n_src << 4; k < L; ++k) c = T[0][(c ^ src[k]) & 255u] ^ (c >> 8);
        v ^= c;
    }
    for (int o = 32; o; o >>= 1) v ^= __shfl_xor( v, o, 64 );
    if ((t & 63u) == 0u) part[t >> 6] = v;
    __syncthreads();
    if (t == 0u)
    {
        const uint32_t crc = part[0] ^ part[1] ^ part[2] ^ part[3] ^ 0xFFFFFFFFu;
        uint8_t* trailer = dst + L;
        for (uint32_t k = 0; k < 4u; ++k) { trailer[k] = (uint8_t)(crc >> (8u * k)); trailer[4u + k] = (uint8_t)(L >> (8u * k)); }
    }
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_bam_format_temp_bytes(uint32_t n, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    NVB_REQUIRE( n < 0x7FFFFFFFu, "n too large" );
    *bytes = bam_scan_bytes( n ) + 8u;                                         // a host formula: the same on every device, and known without one
    return NVBIO_OK;
}

nvbio_status nvbio_bam_record_offsets(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, uint64_t* offsets_dev,
                                      void* temp_dev, uint64_t temp_bytes, void* stream)
{
    BamPlan plan; NVB_CHECK( bam_plan( refs, records, flags, NVBIO_BAM_LENGTHS_ONLY | NVBIO_BAM_REG2BIN, &plan ) );
    NVB_REQUIRE( offsets_dev != nullptr, "offsets_dev is NULL" );
    const uint32_t n = records->n;
    NVB_REQUIRE( n == 0u || temp_dev != nullptr, "temp_dev is NULL" );
    const uint64_t skip = (8u - ((uintptr_t)temp_dev & 7u)) & 7u;
    NVB_REQUIRE( n == 0u || (flags & NVBIO_BAM_LENGTHS_ONLY) || temp_bytes >= bam_scan_bytes( n ) + 8u, "temp_bytes too small (nvbio_bam_format_temp_bytes)" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0u) { NVB_HIP( hipMemsetAsync( offsets_dev, 0, sizeof(uint64_t), s ) ); return NVBIO_OK; }
    NVB_CHECK( with_value( BamLdsBytes(), (int)plan.lds, [&](auto L) {
        constexpr int LDS = decltype(L)::value, G = BamGroups<LDS>::value;
        const dim3 grid( (unsigned)(((uint64_t)n + 1u + (G - 1)) / G) );
        return NVB_LAUNCH( (bam_lengths_kernel<LDS>), grid, dim3(16 * G), s, *refs, *records, flags, plan.stage, offsets_dev );
    }, []() { set_error( "bam: no kernel for this LDS size" ); return NVBIO_ERR_UNSUPPORTED; } ) );
    if (flags & NVBIO_BAM_LENGTHS_ONLY) return NVBIO_OK;
    uint64_t* sums = (uint64_t*)((uint8_t*)temp_dev + skip);
    const uint32_t tiles = (uint32_t)(bam_scan_bytes( n ) / 8u);
    NVB_CHECK( NVB_LAUNCH( bam_tile_sums_kernel, dim3(tiles), dim3(256), s, offsets_dev, n + 1u, sums ) );
    NVB_CHECK( NVB_LAUNCH( bam_scan_sums_kernel, dim3(1), dim3(1024), s, sums, tiles ) );
    return NVB_LAUNCH( bam_tile_scan_kernel, dim3(tiles), dim3(256), s, offsets_dev, n + 1u, (const uint64_t*)sums );
}

nvbio_status nvbio_bam_format(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, const uint64_t* offsets_dev,
                              uint8_t* data_dev, uint64_t data_capacity, uint32_t* n_skipped_dev, uint32_t* status_dev, void* stream)
{
    BamPlan plan; NVB_CHECK( bam_plan( refs, records, flags, NVBIO_BAM_REG2BIN, &plan ) );
    NVB_REQUIRE( n_skipped_dev != nullptr && status_dev != nullptr, "n_skipped_dev or status_dev is NULL" );
    const uint32_t n = records->n;
    NVB_REQUIRE( n == 0u || offsets_dev != nullptr, "offsets_dev is NULL" );
    NVB_REQUIRE( n == 0u || data_capacity == 0u || data_dev != nullptr, "data_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)data_dev & 15u) == 0u, "data_dev must be 16-byte aligned" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    NVB_HIP( hipMemsetAsync( n_skipped_dev, 0, sizeof(uint32_t), s ) );
    if (n == 0u) return NVBIO_OK;
    return with_value( BamLdsBytes(), (int)plan.lds, [&](auto L) {
        constexpr int LDS = decltype(L)::value, G = BamGroups<LDS>::value;
        const dim3 grid( (unsigned)(((uint64_t)n + (G - 1)) / G) );
        return NVB_LAUNCH( (bam_write_kernel<LDS>), grid, dim3(16 * G), s, *refs, *records, flags, plan.stage, offsets_dev, data_dev, data_capacity,
                           n_skipped_dev, status_dev );
    }, []() { set_error( "bam: no kernel for this LDS size" ); return NVBIO_ERR_UNSUPPORTED; } );
}

nvbio_status nvbio_bgzf_framed_bytes(uint64_t n_bytes, uint64_t* framed_bytes)
{
    NVB_REQUIRE( framed_bytes != nullptr, "framed_bytes is NULL" );
    NVB_REQUIRE( n_bytes < (1ull << 46), "n_bytes too large" );
    *framed_bytes = n_bytes + (uint64_t)NVBIO_BGZF_OVERHEAD * ((n_bytes + NVBIO_BGZF_BLOCK_BYTES - 1u) / NVBIO_BGZF_BLOCK_BYTES);
    return NVBIO_OK;
}

nvbio_status nvbio_bgzf_frame(int device, const uint8_t* data_dev, uint64_t n_bytes, uint8_t* out_dev, uint64_t out_capacity, void* stream)
{
    uint64_t framed = 0; NVB_CHECK( nvbio_bgzf_framed_bytes( n_bytes, &framed ) );
    NVB_REQUIRE( n_bytes == 0u || (data_dev != nullptr && out_dev != nullptr), "data_dev or out_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)data_dev & 15u) == 0u && ((uintptr_t)out_dev & 15u) == 0u, "data_dev and out_dev must be 16-byte aligned" );
    NVB_REQUIRE( out_capacity >= framed, "out_capacity is below nvbio_bgzf_framed_bytes( n_bytes )" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    if (n_bytes == 0u) return NVBIO_OK;
    const dim3 grid( (unsigned)((n_bytes + NVBIO_BGZF_BLOCK_BYTES - 1u) / NVBIO_BGZF_BLOCK_BYTES) );
    return NVB_LAUNCH( bgzf_frame_kernel, grid, dim3(256), (hipStream_t)stream, data_dev, n_bytes, out_dev, bgzf_consts() );
}

} // extern "C"
