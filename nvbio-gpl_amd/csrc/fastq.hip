// fastq.hip -- FASTQ text parsed on the device (gfx950) into an io::SequenceData<DNA_N>-shaped batch:
//         SequenceDataFile_FASTQ_parser::nextChunk, get                 nvbio/io/sequence/sequence_fastq.cpp:39-203, sequence_fastq.h:123-137
//         SequenceDataEncoder::push_back, nst_nt4, the quality tables   nvbio/io/sequence/sequence_encoder.cpp:30-107,304-368
// The reference parses on the host, one byte at a time, and encodes one read at a time.  Its grammar (the table in nvbio_amd.h) is one
// sequential machine: a record boundary cannot be found locally, since a quality line may begin with '@' and hold '+'.  A byte is a
// FUNCTION over the machine's six states (GAP NAME SEQ PLUS QUAL and the absorbing ERR), six 3-bit fields of one register, and functions
// compose associatively: (f then g)[s] = g[f[s]].  So the state in front of every byte comes from a scan:
//
//   nvbio_fastq_scan
//     fastq_tile_fn_kernel         one workgroup per 4096-byte tile: each lane composes its 16 bytes (one 16-byte load), lanes scan across the
//                                  wave with cross-lane moves, waves through LDS; the tile's function goes to tile_fn[tile]
//     fastq_tile_scan_kernel<1>    ONE workgroup scans tile_fn in place: tile_fn[t] = the function of everything before tile t
//     fastq_apply_kernel<0>        each lane now knows its state; counts the record ends (QUAL -> GAP) of its tile
//     fastq_tile_scan_kernel<0>    ONE workgroup sums the counts in place
//     fastq_apply_kernel<1>        the same walk: a '@' read in GAP starts the record whose number is the count of ends before it
//                                  (starts and ends alternate, and ERR ends nothing, so nothing behind a marker error is a record);
//                                  writes rec_start[], the error's offset, the end of record max_records - 1, the unfinished record's '@'
//     fastq_lengths_kernel         one wave per record finds its fields with ballots from its '@' on: name length, kept symbols, quality
//                                  length -> lens[] = name length << 32 | min( quality length, truncate_len ); status bits and maxima
//     hipcub ExclusiveSum          of lens[i < n_records] (one uint64 scan gives both indices: a text has less than 2^32 bytes)
//     fastq_summary_kernel         *summary_dev
//   nvbio_fastq_encode
//     fastq_zero_words_kernel      the ceil( n_symbols / 8 ) words
//     fastq_encode_kernel          one wave per record: names and qualities as striped bytes; the kept symbols of a (multi-line)
//                                  sequence are compacted with ballot and popcount into a window of the wave's LDS, from which each lane
//                                  assembles whole words: a word inside the window's symbol range is a plain store, the word at either
//                                  end, which a neighbouring read (or the next window of a long read) may share, an atomicOr
// No workgroup waits on another inside a launch.  Offsets into the text are 32-bit: a text of 2^32 bytes or more is refused.
#include "byte_scan.h"
#include <hipcub/hipcub.hpp>

namespace nvbio_amd {

enum : uint32_t { FQ_GAP = 0u, FQ_NAME = 1u, FQ_SEQ = 2u, FQ_PLUS = 3u, FQ_QUAL = 4u, FQ_ERR = 5u };
static constexpr uint32_t FQ_TILE = BS_TILE;
static constexpr uint32_t FQ_WIN  = 1024u;                     // symbols of a read staged in a wave's LDS at a time
static constexpr uint32_t FQ_MIN_RECORD = 5u;                  // '@' and the four bytes that end its fields

constexpr uint32_t fq_fn(uint32_t gap, uint32_t name, uint32_t seq, uint32_t plus, uint32_t qual)
{
    return gap | (name << 3) | (seq << 6) | (plus << 9) | (qual << 12) | (FQ_ERR << 15);
}
// the grammar, one function per byte class (sequence_fastq.cpp:55-75, :79, :103-107, :129, :144)
static constexpr uint32_t FQ_ID  = fq_fn( FQ_GAP,  FQ_NAME, FQ_SEQ,  FQ_PLUS, FQ_QUAL );    // ' ', and the padding behind the text
static constexpr uint32_t FQ_NL  = fq_fn( FQ_GAP,  FQ_SEQ,  FQ_SEQ,  FQ_QUAL, FQ_GAP  );
static constexpr uint32_t FQ_AT  = fq_fn( FQ_NAME, FQ_NAME, FQ_SEQ,  FQ_PLUS, FQ_QUAL );
static constexpr uint32_t FQ_PL  = fq_fn( FQ_ERR,  FQ_NAME, FQ_PLUS, FQ_PLUS, FQ_QUAL );
static constexpr uint32_t FQ_NUL = fq_fn( FQ_ERR,  FQ_SEQ,  FQ_PLUS, FQ_QUAL, FQ_GAP  );
static constexpr uint32_t FQ_OTH = fq_fn( FQ_ERR,  FQ_NAME, FQ_SEQ,  FQ_PLUS, FQ_QUAL );

// what the scan leaves for the calls behind it
struct FqInfo
{
    uint32_t final_state;       // the machine's state behind the whole text
    uint32_t total_ends;        // records that end inside the text, before any marker error
    uint32_t has_err, err_off, err_char;
    uint32_t cap_end;           // the offset behind the byte that ended record max_records - 1
    uint32_t last_start;        // the '@' of the record that does not end
    uint32_t pad;
};

__device__ __forceinline__ uint32_t fq_byte_fn(const uint32_t c)
{
    return c == '\n' ? FQ_NL : c == ' ' ? FQ_ID : c == '@' ? FQ_AT : c == '+' ? FQ_PL : c == 0u ? FQ_NUL : FQ_OTH;
}
__device__ __forceinline__ uint32_t fq_next(const uint32_t s, const uint32_t c) { return (fq_byte_fn( c ) >> (3u * s)) & 7u; }
__device__ __forceinline__ bool fq_is_graph(const uint32_t c) { return c >= 0x21u && c <= 0x7Eu; }
__device__ __forceinline__ bool fq_ends_line(const uint32_t c) { return c == '\n' || c == 0u; }

__device__ __forceinline__ void fq_wave_sync()
{
    __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
}

// the 16 bytes of this lane: text[at, at + 16), spaces (the identity) behind the text
__device__ __forceinline__ void fq_load16(const uint8_t* __restrict__ text, const uint32_t n, const uint64_t at, uint32_t w[4]) { bs_load16( text, n, at, 0x20202020u, w ); }
__device__ __forceinline__ uint32_t fq_fn16(const uint32_t w[4])
{
    uint32_t f = FQ_ID;
#pragma unroll
    for (uint32_t k = 0u; k < 16u; ++k) f = bs_compose( f, fq_byte_fn( bs_byte( w, k ) ) );
    return f;
}

// ---- the function of every tile ----
__global__ void __launch_bounds__(256)
fastq_tile_fn_kernel(const uint8_t* __restrict__ text, const uint32_t n, uint32_t* __restrict__ tile_fn)
{
    __shared__ uint32_t lds4[4];
    uint32_t w[4], total;
    fq_load16( text, n, (uint64_t)blockIdx.x * FQ_TILE + threadIdx.x * 16u, w );
    (void)bs_block_prefix( fq_fn16( w ), lds4, &total );
    if (threadIdx.x == 0u) tile_fn[blockIdx.x] = total;
}

// ---- one workgroup's exclusive scan of vals[0, n) in place: COMPOSE: functions (*total = the state GAP ends in), else sums ----
template <bool COMPOSE>
__global__ void __launch_bounds__(1024)
fastq_tile_scan_kernel(uint32_t* __restrict__ vals, const uint32_t n, uint32_t* __restrict__ total)
{
    __shared__ uint32_t part[16];
    const uint32_t tot = bs_scan_in_place( vals, n, COMPOSE ? BS_IDENTITY : 0u,
                                           [](const uint32_t a, const uint32_t b) -> uint32_t { return COMPOSE ? bs_compose( a, b ) : a + b; }, part );
    if (threadIdx.x == 0u) *total = COMPOSE ? (tot & 7u) : tot;
}

// ---- the walk over every byte with its state known.  EMIT = 0: tile_ends[tile] = the record ends in the tile.  EMIT = 1 (tile_ends
//      scanned): the records' starts and the offsets the summary needs ----
template <bool EMIT>
__global__ void __launch_bounds__(256)
fastq_apply_kernel(const uint8_t* __restrict__ text, const uint32_t n, const uint32_t* __restrict__ tile_fn, uint32_t* __restrict__ tile_ends,
                   const uint32_t max_records, const uint32_t cap, uint32_t* __restrict__ rec_start, FqInfo* __restrict__ info)
{
    __shared__ uint32_t lds4[4], cnt4[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t at = (uint64_t)blockIdx.x * FQ_TILE + threadIdx.x * 16u;
    uint32_t w[4], total;
    fq_load16( text, n, at, w );
    const uint32_t ex = bs_block_prefix( fq_fn16( w ), lds4, &total );
    const uint32_t s0 = (ex >> (3u * (tile_fn[blockIdx.x] & 7u))) & 7u;       // GAP through everything before the tile, then through the lanes before

    uint32_t s = s0, ends = 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 16u; ++k)
    {
        const uint32_t c = bs_byte( w, k );
        ends += (s == FQ_QUAL && fq_ends_line( c ) && at + k < n) ? 1u : 0u;
        s = fq_next( s, c );
    }
    uint32_t inc = ends;
    for (uint32_t o = 1u; o < 64u; o <<= 1) { const uint32_t t = __shfl_up( inc, o, 64 ); if (lane >= o) inc += t; }
    if (lane == 63u) cnt4[wave] = inc;
    __syncthreads();
    uint32_t before = inc - ends, tile_total = 0u;
    for (uint32_t v = 0u; v < 4u; ++v) { const uint32_t t = cnt4[v]; if (v < wave) before += t; tile_total += t; }
    if (!EMIT) { if (threadIdx.x == 0u) tile_ends[blockIdx.x] = tile_total; return; }

    uint32_t e = tile_ends[blockIdx.x] + before;                             // the record ends before this lane's first byte
    const uint32_t total_ends = info->total_ends;
    s = s0;
#pragma unroll
    for (uint32_t k = 0u; k < 16u; ++k)
    {
        const uint32_t c = bs_byte( w, k );
        if (at + k < n)
        {
            const uint32_t p = (uint32_t)(at + k);
            if (s == FQ_GAP)
            {
                if (c == '@')
                {
                    if (e < cap) rec_start[e] = p;
                    if (e == total_ends) info->last_start = p;
                }
                else if (c != '\n' && c != ' ') { info->has_err = 1u; info->err_off = p; info->err_char = c; }
            }
            else if (s == FQ_QUAL && fq_ends_line( c ))
            {
                if (e + 1u == max_records) info->cap_end = p + 1u;
                ++e;
            }
        }
        s = fq_next( s, c );
    }
}

// ---- a record's fields, found by its wave from its '@' on ----
struct FqFields { uint32_t name_begin, name_len, seq_begin, seq_end, kept, qual_begin, qual_len; };

// the first byte of text[from, n) that ends the field -- '+' or NUL when `plus`, '\n' or NUL otherwise -- and *kept = the bytes
// 0x21..0x7E before it; n when there is none.  Wave-uniform.
__device__ __forceinline__ uint32_t fq_field_end(const uint8_t* __restrict__ text, const uint32_t n, const uint32_t from, const uint32_t lane,
                                                 const bool plus, uint32_t* kept)
{
    uint32_t k = 0u;
    for (uint64_t at = from; at < n; at += 64u)
    {
        const uint64_t p = at + lane;
        const uint32_t c = p < n ? (uint32_t)text[p] : 0x100u;
        const uint64_t tm = __ballot( plus ? (c == '+' || c == 0u) : (c == '\n' || c == 0u) ), gm = __ballot( fq_is_graph( c ) );
        if (tm)
        {
            const uint32_t z = (uint32_t)__builtin_ctzll( tm );
            *kept = k + (uint32_t)__popcll( gm & ((1ull << z) - 1ull) );
            return (uint32_t)(at + z);
        }
        k += (uint32_t)__popcll( gm );
    }
    *kept = k;
    return n;
}
__device__ __forceinline__ FqFields fq_fields(const uint8_t* __restrict__ text, const uint32_t n, const uint32_t start, const uint32_t lane)
{
    auto behind = [n](const uint32_t x) -> uint32_t { return x < n ? x + 1u : n; };
    FqFields f;
    uint32_t unused;
    f.name_begin = behind( start );
    const uint32_t name_end = fq_field_end( text, n, f.name_begin, lane, false, &unused );
    f.name_len  = name_end - f.name_begin;
    f.seq_begin = behind( name_end );
    f.seq_end   = fq_field_end( text, n, f.seq_begin, lane, true, &f.kept );
    const uint32_t plus_end = fq_field_end( text, n, behind( f.seq_end ), lane, false, &unused );
    f.qual_begin = behind( plus_end );
    f.qual_len   = fq_field_end( text, n, f.qual_begin, lane, false, &unused ) - f.qual_begin;
    return f;
}

__device__ __forceinline__ uint32_t fq_min(const uint32_t a, const uint32_t b) { return a < b ? a : b; }

// ---- lens[i] = name length << 32 | read length of record i < n_records; the maxima and the LENGTH / EMPTY bits into *summary ----
__global__ void __launch_bounds__(256)
fastq_lengths_kernel(const uint8_t* __restrict__ text, const uint32_t n, const nvbio_fastq_params params, const FqInfo* __restrict__ info,
                     const uint32_t* __restrict__ rec_start, uint64_t* __restrict__ lens, nvbio_fastq_summary* __restrict__ summary)
{
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane( threadIdx.x >> 6 );
    const uint32_t n_rec = fq_min( info->total_ends, params.max_records ), n_waves = gridDim.x * 4u;
    uint32_t max_read = 0u, max_name = 0u, status = 0u, bad = 0xFFFFFFFFu;
    for (uint32_t i = blockIdx.x * 4u + wave; i < n_rec; i += n_waves)
    {
        const FqFields f = fq_fields( text, n, rec_start[i], lane );
        const uint32_t len = fq_min( f.qual_len, params.truncate_len );
        if (lane == 0u) lens[i] = ((uint64_t)f.name_len << 32) | len;
        max_read = len > max_read ? len : max_read;
        max_name = f.name_len > max_name ? f.name_len : max_name;
        if (f.qual_len != f.kept) { status |= NVBIO_FASTQ_STATUS_LENGTH; bad = fq_min( bad, i ); }
        if (f.qual_len == 0u)     { status |= NVBIO_FASTQ_STATUS_EMPTY;  bad = fq_min( bad, i ); }
    }
    if (lane == 0u)
    {
        if (max_read) atomicMax( &summary->max_read_len, max_read );
        if (max_name) atomicMax( &summary->max_name_len, max_name );
        if (status)   atomicOr( &summary->status, status );
        if (bad != 0xFFFFFFFFu) atomicMin( &summary->first_bad_record, bad );
    }
}

// lens[i] for a record, 0 behind the last: what the scan over the capacity reads
struct FqLenAt
{
    const uint64_t* lens;
    const FqInfo*   info;
    uint32_t        max_records;
    __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t i) const
    {
        const uint32_t t = info->total_ends;
        return i < (t < max_records ? t : max_records) ? lens[i] : 0ull;
    }
};
using FqLenIterator = hipcub::TransformInputIterator<uint64_t, FqLenAt, hipcub::CountingInputIterator<uint32_t>>;

__global__ void fastq_init_kernel(FqInfo* __restrict__ info, nvbio_fastq_summary* __restrict__ summary)
{
    *info = FqInfo{ FQ_GAP, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    *summary = nvbio_fastq_summary{ 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu };
}

__global__ void fastq_summary_kernel(const uint32_t n, const uint32_t max_records, const FqInfo* __restrict__ info, const uint64_t* __restrict__ index64,
                                     nvbio_fastq_summary* __restrict__ summary)
{
    const uint32_t n_rec = fq_min( info->total_ends, max_records );
    const uint64_t total = index64[n_rec];
    summary->n_records    = n_rec;
    summary->n_symbols    = (uint32_t)total;
    summary->n_name_bytes = (uint32_t)(total >> 32);
    if (info->total_ends >= max_records) summary->consumed_bytes = max_records ? info->cap_end : 0u;   // the machine stopped there
    else if (info->has_err)
    {
        summary->status |= NVBIO_FASTQ_STATUS_MARKER;
        summary->consumed_bytes = summary->error_offset = info->err_off;
        summary->error_char = info->err_char;
    }
    else if (info->final_state != FQ_GAP) { summary->status |= NVBIO_FASTQ_STATUS_INCOMPLETE; summary->consumed_bytes = info->last_start; }
    else summary->consumed_bytes = n;
}

// ---- encode ----
__global__ void __launch_bounds__(256)
fastq_zero_words_kernel(const uint32_t max_records, const FqInfo* __restrict__ info, const uint64_t* __restrict__ index64, uint32_t* __restrict__ reads4,
                        const uint64_t capacity_words)
{
    const uint64_t used = ((uint64_t)(uint32_t)index64[fq_min( info->total_ends, max_records )] + 7u) >> 3;
    const uint64_t words = used < capacity_words ? used : capacity_words;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256u) reads4[i] = 0u;
}

__device__ __forceinline__ uint32_t fq_symbol(const uint32_t c)                   // nst_nt4 (sequence_encoder.cpp:30-47)
{
    const uint32_t u = c & ~0x20u;                                                 // 'a' -> 'A'; '-' (0x2D) -> 0x0D, which no other kept byte maps to
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : c == '-' ? 5u : 4u;
}
static __device__ const uint8_t FQ_SOLEXA_LOW[20] = { 0, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10 };     // s_solexa_to_phred below 20; q - 10 from there
__device__ __forceinline__ uint8_t fq_quality(const uint32_t q, const uint32_t encoding)           // convert_to_phred_quality (:53-107)
{
    if (encoding == NVBIO_FASTQ_PHRED33) return (uint8_t)(q - 33u);
    if (encoding == NVBIO_FASTQ_PHRED64) return (uint8_t)(q - 64u);
    if (encoding == NVBIO_FASTQ_SOLEXA) return (uint8_t)(q < 20u ? FQ_SOLEXA_LOW[q] : q - 10u);
    return (uint8_t)q;
}

__global__ void __launch_bounds__(256)
fastq_encode_kernel(const uint8_t* __restrict__ text, const uint32_t n, const nvbio_fastq_params params, const FqInfo* __restrict__ info,
                    const uint32_t* __restrict__ rec_start, const uint64_t* __restrict__ index64, uint32_t* __restrict__ reads4, const uint64_t capacity_symbols,
                    uint32_t* __restrict__ read_index, uint8_t* __restrict__ quals, uint8_t* __restrict__ names, const uint64_t names_capacity,
                    uint32_t* __restrict__ name_index, uint32_t* __restrict__ status)
{
    __shared__ uint8_t stage[4][FQ_WIN];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane( threadIdx.x >> 6 );
    const uint32_t n_rec = fq_min( info->total_ends, params.max_records ), n_waves = gridDim.x * 4u;
    const bool rev = (params.strand_op & NVBIO_FASTQ_REVERSE_OP) != 0u, comp = (params.strand_op & NVBIO_FASTQ_COMPLEMENT_OP) != 0u;
    uint8_t* buf = stage[wave];
    for (uint32_t i = blockIdx.x * 4u + wave; i <= n_rec; i += n_waves)
    {
        const uint64_t a = index64[i];
        const uint32_t r0 = (uint32_t)a, q0 = (uint32_t)(a >> 32);
        if (lane == 0u) { read_index[i] = r0; name_index[i] = q0; }
        if (i == n_rec) break;
        const uint64_t z = index64[i + 1u];
        const uint32_t r1 = (uint32_t)z, q1 = (uint32_t)(z >> 32), len = r1 - r0, name_len = q1 - q0;
        if (r1 > capacity_symbols || q1 > names_capacity) { if (lane == 0u) atomicOr( status, NVBIO_FASTQ_STATUS_CAPACITY ); continue; }
        const FqFields f = fq_fields( text, n, rec_start[i], lane );

        for (uint32_t k = lane; k < name_len; k += 64u) names[q0 + k] = text[f.name_begin + k];
        if (quals)
            for (uint32_t k = lane; k < len; k += 64u) quals[r0 + k] = fq_quality( text[f.qual_begin + (rev ? len - 1u - k : k)], params.quality_encoding );

        // symbol j of the read is the j-th kept byte of text[seq_begin, seq_end), 4 from the kept bytes' end on; it is stored at k = j, or len - 1 - j
        uint32_t pos = f.seq_begin, jb = 0u;                                   // jb: the kept bytes before pos
        for (uint32_t b = 0u; b < len; b += FQ_WIN)
        {
            const uint32_t e = len - b > FQ_WIN ? b + FQ_WIN : len;
            for (uint32_t k = lane; k < e - b; k += 64u) buf[k] = 4u;
            fq_wave_sync();
            while (pos < f.seq_end && jb < e)
            {
                const uint64_t p = (uint64_t)pos + lane;
                const uint32_t c = p < f.seq_end ? (uint32_t)text[p] : 0u;
                const bool g = fq_is_graph( c );
                const uint64_t m = __ballot( g );
                const uint32_t j = jb + (uint32_t)__popcll( m & ((1ull << lane) - 1ull) ), cnt = (uint32_t)__popcll( m );
                if (g && j >= b && j < e) buf[j - b] = (uint8_t)fq_symbol( c );
                if (cnt > e - jb) break;                                        // the rest of these 64 bytes belongs to the next window: read again then
                jb += cnt;
                pos = f.seq_end - pos > 64u ? pos + 64u : f.seq_end;
            }
            fq_wave_sync();
            const uint32_t g0 = r0 + (rev ? len - e : b), g1 = r0 + (rev ? len - b : e);     // the window's symbols in the stream
            for (uint32_t w = (g0 >> 3) + lane; w <= ((g1 - 1u) >> 3); w += 64u)
            {
                uint32_t word = 0u;
#pragma unroll
                for (uint32_t t = 0u; t < 8u; ++t)
                {
                    const uint32_t g = w * 8u + t;
                    if (g >= g0 && g < g1)
                    {
                        const uint32_t k = g - r0;
                        uint32_t c = buf[(rev ? len - 1u - k : k) - b];
                        if (comp) c = c < 4u ? 3u - c : 4u;
                        word |= c << (28u - 4u * t);
                    }
                }
                if (w * 8u >= g0 && w * 8u + 8u <= g1) reads4[w] = word;
                else                                   atomicOr( &reads4[w], word );
            }
            fq_wave_sync();
        }
    }
}

// ---- the temp of both calls, laid out once ----
struct FqTemp
{
    FqInfo*   info;
    uint32_t* tile_fn;
    uint32_t* tile_ends;
    uint32_t* rec_start;
    uint64_t* lens;
    uint64_t* index64;
    uint8_t*  work;
    uint32_t  n_tiles, cap;
    size_t    work_bytes;
    uint64_t  bytes;
};

static nvbio_status fastq_temp(const uint64_t text_bytes, const uint32_t max_records, uint8_t* base, FqTemp* t)
{
    t->n_tiles = (uint32_t)((text_bytes + FQ_TILE - 1u) / FQ_TILE);
    const uint64_t most = text_bytes / FQ_MIN_RECORD;
    t->cap = (uint32_t)(max_records < most ? max_records : most);
    t->work_bytes = 0;
    FqLenIterator it( hipcub::CountingInputIterator<uint32_t>( 0u ), FqLenAt{ nullptr, nullptr, 0u } );
    NVB_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, t->work_bytes, it, (uint64_t*)nullptr, (int)(t->cap + 1u), (hipStream_t)0 ) );
    ScratchLayout l( base );
    t->info      = l.take<FqInfo>( 1u );
    t->tile_fn   = l.take<uint32_t>( t->n_tiles );
    t->tile_ends = l.take<uint32_t>( t->n_tiles );
    t->rec_start = l.take<uint32_t>( t->cap );
    t->lens      = l.take<uint64_t>( t->cap );
    t->index64   = l.take<uint64_t>( (uint64_t)t->cap + 1u );
    t->work      = l.take<uint8_t>( t->work_bytes );
    t->bytes     = l.bytes();
    return NVBIO_OK;
}

// the checks of both calls that need no device
static nvbio_status fastq_check(const uint8_t* text_dev, const uint64_t text_bytes, const nvbio_fastq_params* params, const void* temp_dev,
                                const uint64_t temp_bytes, FqTemp* t)
{
    NVB_REQUIRE( params != nullptr, "params is NULL" );
    NVB_REQUIRE( params->quality_encoding <= NVBIO_FASTQ_SOLEXA, "quality_encoding must be NVBIO_FASTQ_PHRED .. NVBIO_FASTQ_SOLEXA" );
    NVB_REQUIRE( params->strand_op <= NVBIO_FASTQ_REVERSE_COMPLEMENT_OP, "strand_op must be NVBIO_FASTQ_NO_OP .. NVBIO_FASTQ_REVERSE_COMPLEMENT_OP" );
    if (text_bytes >= (1ull << 32))
    {
        set_error( "fastq: a text of %llu bytes: offsets into the text are 32-bit, feed chunks below 4 GiB", (unsigned long long)text_bytes );
        return NVBIO_ERR_UNSUPPORTED;
    }
    NVB_REQUIRE( text_bytes == 0u || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)text_dev & 15u) == 0u, "text_dev must be 16-byte aligned" );
    NVB_REQUIRE( temp_dev != nullptr, "temp_dev is NULL" );
    uint8_t* base = (uint8_t*)(((uintptr_t)temp_dev + 255u) & ~(uintptr_t)255u);
    NVB_CHECK( fastq_temp( text_bytes, params->max_records, base, t ) );
    NVB_REQUIRE( temp_bytes >= (uint64_t)(base - (uint8_t*)temp_dev) + ScratchLayout::round( t->bytes - 256u ), "temp_bytes too small (nvbio_fastq_temp_bytes)" );
    return NVBIO_OK;
}

static unsigned fastq_record_grid(const uint32_t cap) { return grid_for( ((uint64_t)cap + 1u + 3u) / 4u, 1u, 8192u ); }

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_fastq_temp_bytes(uint64_t text_bytes, uint32_t max_records, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    if (text_bytes >= (1ull << 32))
    {
        set_error( "fastq: a text of %llu bytes: offsets into the text are 32-bit, feed chunks below 4 GiB", (unsigned long long)text_bytes );
        return NVBIO_ERR_UNSUPPORTED;
    }
    FqTemp t; NVB_CHECK( fastq_temp( text_bytes, max_records, nullptr, &t ) );
    *bytes = t.bytes;
    return NVBIO_OK;
}

nvbio_status nvbio_fastq_scan(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fastq_params* params, nvbio_fastq_summary* summary_dev,
                              void* temp_dev, uint64_t temp_bytes, void* stream)
{
    FqTemp t; NVB_CHECK( fastq_check( text_dev, text_bytes, params, temp_dev, temp_bytes, &t ) );
    NVB_REQUIRE( summary_dev != nullptr, "summary_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)text_bytes;
    NVB_CHECK( NVB_LAUNCH( fastq_init_kernel, dim3(1), dim3(1), s, t.info, summary_dev ) );
    if (t.n_tiles)
    {
        NVB_CHECK( NVB_LAUNCH( fastq_tile_fn_kernel, dim3(t.n_tiles), dim3(256), s, text_dev, n, t.tile_fn ) );
        NVB_CHECK( NVB_LAUNCH( fastq_tile_scan_kernel<true>, dim3(1), dim3(1024), s, t.tile_fn, t.n_tiles, &t.info->final_state ) );
        NVB_CHECK( NVB_LAUNCH( fastq_apply_kernel<false>, dim3(t.n_tiles), dim3(256), s, text_dev, n, t.tile_fn, t.tile_ends, params->max_records, t.cap,
                               t.rec_start, t.info ) );
        NVB_CHECK( NVB_LAUNCH( fastq_tile_scan_kernel<false>, dim3(1), dim3(1024), s, t.tile_ends, t.n_tiles, &t.info->total_ends ) );
        NVB_CHECK( NVB_LAUNCH( fastq_apply_kernel<true>, dim3(t.n_tiles), dim3(256), s, text_dev, n, t.tile_fn, t.tile_ends, params->max_records, t.cap,
                               t.rec_start, t.info ) );
        if (t.cap)
            NVB_CHECK( NVB_LAUNCH( fastq_lengths_kernel, dim3(fastq_record_grid( t.cap )), dim3(256), s, text_dev, n, *params, t.info, t.rec_start, t.lens,
                                   summary_dev ) );
    }
    FqLenIterator it( hipcub::CountingInputIterator<uint32_t>( 0u ), FqLenAt{ t.lens, t.info, params->max_records } );
    size_t work = t.work_bytes;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum( t.work, work, it, t.index64, (int)(t.cap + 1u), s );
    if (e != hipSuccess) { set_error( "fastq_scan: scan failed: %s", hipGetErrorString( e ) ); return NVBIO_ERR_HIP; }
    return NVB_LAUNCH( fastq_summary_kernel, dim3(1), dim3(1), s, n, params->max_records, t.info, t.index64, summary_dev );
}

nvbio_status nvbio_fastq_encode(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fastq_params* params, const void* temp_dev,
                                uint64_t temp_bytes, uint32_t* reads4_dev, uint64_t reads4_capacity_words, uint32_t* read_index_dev, uint8_t* quals_dev,
                                uint8_t* names_dev, uint64_t names_capacity, uint32_t* name_index_dev, uint32_t* status_dev, void* stream)
{
    FqTemp t; NVB_CHECK( fastq_check( text_dev, text_bytes, params, temp_dev, temp_bytes, &t ) );
    NVB_REQUIRE( read_index_dev != nullptr && name_index_dev != nullptr && status_dev != nullptr, "read_index_dev, name_index_dev or status_dev is NULL" );
    NVB_REQUIRE( reads4_capacity_words == 0u || reads4_dev != nullptr, "reads4_dev is NULL" );
    NVB_REQUIRE( names_capacity == 0u || names_dev != nullptr, "names_dev is NULL" );
    NVB_REQUIRE( reads4_capacity_words < (1ull << 29), "reads4_capacity_words must be below 2^29 (2^32 symbols)" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (reads4_capacity_words)
        NVB_CHECK( NVB_LAUNCH( fastq_zero_words_kernel, dim3(grid_for( reads4_capacity_words )), dim3(256), s, params->max_records, t.info, t.index64,
                               reads4_dev, reads4_capacity_words ) );
    return NVB_LAUNCH( fastq_encode_kernel, dim3(fastq_record_grid( t.cap )), dim3(256), s, text_dev, (uint32_t)text_bytes, *params, t.info, t.rec_start,
                       t.index64, reads4_dev, reads4_capacity_words * 8u, read_index_dev, quals_dev, names_dev, names_capacity, name_index_dev, status_dev );
}

} // extern "C"
