// fasta.hip -- reference FASTA text turned on the device (gfx950) into the 2-bit packed text, the sequence and hole tables and the names:
//         FASTA_inc_reader::read, get                      nvbio/fasta/fasta_inl.h:64-122
//         nvBWT's Writer, nst_nt4_table, rand_bp           nvBWT/nvBWT.cu:50-195
// The reference runs this on the host, one byte at a time.  Its grammar (the table in nvbio_amd.h) is one sequential machine over five
// states, run here as fastq.hip runs its own (byte_scan.h): a byte is a function over the states, functions compose.  There are no
// records to hand to waves: the body is a stream compaction, and everything a byte needs to know is a COUNT of what came before it.
//
//   nvbio_fasta_scan
//     fasta_init_kernel          the state the chunk is entered in, copied into temp (every later launch reads the copy)
//     fasta_tile_fn_kernel       one workgroup per 4096-byte tile: the tile's function
//     fasta_fn_scan_kernel       ONE workgroup: tile_fn[t] = the function of everything before tile t; the state behind the chunk
//     fasta_count_kernel         each lane walks its 16 bytes in its known state: a FaSum per lane (symbols, ambiguous symbols, sequence starts,
//                                hole starts, name bytes, first and last symbol byte), reduced over the tile with fa_combine
//     fasta_sum_scan_kernel      ONE workgroup scans the tiles' FaSum in place; the chunk's totals and *summary_dev
//   nvbio_fasta_encode
//     fasta_zero_kernel          the words no chunk has touched yet
//     fasta_emit_kernel          per tile: symbols staged in LDS in output order; hole starts from the staged neighbour; draws by jumping the
//                                generator; 16 symbols a word; whole words stored 16 bytes at a time, the words at either end of the tile's
//                                range merged with atomicOr
//     fasta_advance_kernel       *state_dev = the scan's copy advanced by the totals
//   nvbio_fasta_finish           one launch closes the tables
// No workgroup waits on another inside a launch.
#include "byte_scan.h"

namespace nvbio_amd {

constexpr uint32_t fa_fn(uint32_t pre, uint32_t id, uint32_t rest, uint32_t body, uint32_t end)
{
    return pre | (id << 3) | (rest << 6) | (body << 9) | (end << 12) | (5u << 15);
}
// the grammar, one function per byte class (fasta_inl.h:73-103)
static constexpr uint32_t FA_GT = fa_fn( NVBIO_FASTA_ID,  NVBIO_FASTA_ID,   NVBIO_FASTA_REST, NVBIO_FASTA_ID,   NVBIO_FASTA_END );
static constexpr uint32_t FA_SP = fa_fn( NVBIO_FASTA_PRE, NVBIO_FASTA_REST, NVBIO_FASTA_REST, NVBIO_FASTA_BODY, NVBIO_FASTA_END );
static constexpr uint32_t FA_NL = fa_fn( NVBIO_FASTA_PRE, NVBIO_FASTA_BODY, NVBIO_FASTA_BODY, NVBIO_FASTA_BODY, NVBIO_FASTA_END );
static constexpr uint32_t FA_FF = fa_fn( NVBIO_FASTA_END, NVBIO_FASTA_ID,   NVBIO_FASTA_REST, NVBIO_FASTA_END,  NVBIO_FASTA_END );
static constexpr uint32_t FA_PAD = 0x41414141u;                // 'A' behind the text: the identity in every state (never counted: the walks stop at n)

static constexpr uint32_t FA_RESET = NVBIO_FASTA_NO_SYMBOL;    // FaSum.first / last: a sequence start
static constexpr uint32_t FA_NOTHING = 0x1FFu;                 //                     neither a symbol nor a sequence start in the segment

enum : uint32_t { FA_EV_NONE = 0u, FA_EV_SYMBOL, FA_EV_START, FA_EV_NAME, FA_EV_END };

__device__ __forceinline__ uint32_t fa_byte_fn(const uint32_t c)
{
    return c == '>' ? FA_GT : c == ' ' ? FA_SP : c == '\n' ? FA_NL : c == 0xFFu ? FA_FF : BS_IDENTITY;
}
__device__ __forceinline__ uint32_t fa_next(const uint32_t s, const uint32_t c) { return (fa_byte_fn( c ) >> (3u * s)) & 7u; }
__device__ __forceinline__ uint32_t fa_fn16(const uint32_t w[4])
{
    uint32_t f = BS_IDENTITY;
#pragma unroll
    for (uint32_t k = 0u; k < 16u; ++k) f = bs_compose( f, fa_byte_fn( bs_byte( w, k ) ) );
    return f;
}
// what byte c, read in state s, is
__device__ __forceinline__ uint32_t fa_event(const uint32_t s, const uint32_t c)
{
    if (s == NVBIO_FASTA_BODY) return c == '>' ? FA_EV_START : c == 0xFFu ? FA_EV_END : (c == '\n' || c == ' ') ? FA_EV_NONE : FA_EV_SYMBOL;
    if (s == NVBIO_FASTA_PRE)  return c == '>' ? FA_EV_START : c == 0xFFu ? FA_EV_END : FA_EV_NONE;
    if (s == NVBIO_FASTA_ID)   return (c == ' ' || c == '\n') ? FA_EV_NONE : FA_EV_NAME;
    return FA_EV_NONE;
}
__device__ __forceinline__ bool fa_is_amb(const uint32_t c)                       // nst_nt4_table[c] >= 4
{
    const uint32_t u = c & ~0x20u;
    return !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
}
__device__ __forceinline__ uint32_t fa_code(const uint32_t c)
{
    const uint32_t u = c & ~0x20u;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : 3u;
}

// ---- drand48: X[i + 1] = (A X[i] + C) mod 2^48.  Affine maps compose, so 2^j steps are one map: 33 of them reach any rank up to 2^32 ----
static constexpr uint64_t FA_LCG_A = 0x5DEECE66Dull, FA_LCG_C = 0xBull, FA_LCG_MASK = (1ull << 48) - 1ull;
struct FaJump { uint64_t a[33], c[33]; };
constexpr FaJump fa_make_jump()
{
    FaJump j{};
    uint64_t a = FA_LCG_A, c = FA_LCG_C;
    for (uint32_t i = 0u; i < 33u; ++i)
    {
        j.a[i] = a; j.c[i] = c;
        c = (a * c + c) & FA_LCG_MASK;                                             // twice the map: a (a x + c) + c
        a = (a * a) & FA_LCG_MASK;
    }
    return j;
}
static __device__ const FaJump FA_JUMP = fa_make_jump();

__device__ __forceinline__ uint64_t fa_lcg_seed(const uint32_t seed) { return ((uint64_t)seed << 16) | 0x330Eull; }
__device__ __forceinline__ uint64_t fa_lcg_step(const uint64_t x) { return (FA_LCG_A * x + FA_LCG_C) & FA_LCG_MASK; }
__device__ __forceinline__ uint64_t fa_lcg_jump(uint64_t x, const uint64_t steps)            // steps <= 2^32
{
    for (uint32_t j = 0u; j < 33u; ++j)
        if ((steps >> j) & 1ull) x = (FA_JUMP.a[j] * x + FA_JUMP.c[j]) & FA_LCG_MASK;
    return x;
}

// ---- what a segment of the text adds, given the state it is entered in.  `hole` counts an ambiguous FIRST symbol as a hole start;
//      fa_combine takes that back when the segment before ends in the same byte.  Associative. ----
struct FaSum { uint32_t sym, amb, seq, hole, name, first, last, pad; };

__device__ __forceinline__ FaSum fa_nothing() { return FaSum{ 0u, 0u, 0u, 0u, 0u, FA_NOTHING, FA_NOTHING, 0u }; }
__device__ __forceinline__ FaSum fa_combine(const FaSum a, const FaSum b)
{
    const uint32_t same = (b.first < 0x100u && fa_is_amb( b.first ) && a.last == b.first) ? 1u : 0u;
    return FaSum{ a.sym + b.sym, a.amb + b.amb, a.seq + b.seq, a.hole + b.hole - same, a.name + b.name,
                  a.first == FA_NOTHING ? b.first : a.first, b.last == FA_NOTHING ? a.last : b.last, 0u };
}
__device__ __forceinline__ FaSum bs_shfl_up(const FaSum v, const uint32_t o)
{
    return FaSum{ (uint32_t)__shfl_up( v.sym, o, 64 ), (uint32_t)__shfl_up( v.amb, o, 64 ), (uint32_t)__shfl_up( v.seq, o, 64 ), (uint32_t)__shfl_up( v.hole, o, 64 ),
                  (uint32_t)__shfl_up( v.name, o, 64 ), (uint32_t)__shfl_up( v.first, o, 64 ), (uint32_t)__shfl_up( v.last, o, 64 ), 0u };
}
__device__ __forceinline__ FaSum fa_shfl_down(const FaSum v, const uint32_t o)
{
    return FaSum{ (uint32_t)__shfl_down( v.sym, o, 64 ), (uint32_t)__shfl_down( v.amb, o, 64 ), (uint32_t)__shfl_down( v.seq, o, 64 ), (uint32_t)__shfl_down( v.hole, o, 64 ),
                  (uint32_t)__shfl_down( v.name, o, 64 ), (uint32_t)__shfl_down( v.first, o, 64 ), (uint32_t)__shfl_down( v.last, o, 64 ), 0u };
}

// what the scan leaves for the calls behind it
struct FaInfo
{
    nvbio_fasta_state snap;     // the state the chunk is entered in
    FaSum    total;             // the chunk's counts, behind snap.last_symbol
    uint32_t final_machine;
    uint32_t end_off;           // the offset of the 0xFF that ended the input
    uint32_t overflow;
    uint32_t pad;
    uint32_t freq[4];           // the encode call's
};
// the segment in front of the chunk, as far as holes go
__device__ __forceinline__ FaSum fa_before(const FaInfo* info) { return FaSum{ 0u, 0u, 0u, 0u, 0u, info->snap.last_symbol, info->snap.last_symbol, 0u }; }

__global__ void fasta_state_init_kernel(nvbio_fasta_state* __restrict__ state, const uint32_t seed)
{
    *state = nvbio_fasta_state{ NVBIO_FASTA_PRE, 0u, 0u, 0u, 0u, 0u, NVBIO_FASTA_NO_SYMBOL, seed, { 0u, 0u, 0u, 0u }, 0u, { 0u, 0u, 0u } };
}

__global__ void fasta_init_kernel(FaInfo* __restrict__ info, const nvbio_fasta_state* __restrict__ state)
{
    info->snap = *state;
    if (info->snap.machine > NVBIO_FASTA_END) info->snap.machine = NVBIO_FASTA_END;          // a state no call here leaves: nothing is read
    info->total = fa_nothing();
    info->final_machine = info->snap.machine;
    info->end_off = 0u;
    info->overflow = 0u;
    info->pad = 0u;
    info->freq[0] = info->freq[1] = info->freq[2] = info->freq[3] = 0u;
}

// ---- the function of every tile ----
__global__ void __launch_bounds__(256)
fasta_tile_fn_kernel(const uint8_t* __restrict__ text, const uint32_t n, uint32_t* __restrict__ tile_fn)
{
    __shared__ uint32_t lds4[4];
    uint32_t w[4], total;
    bs_load16( text, n, (uint64_t)blockIdx.x * BS_TILE + threadIdx.x * 16u, FA_PAD, w );
    (void)bs_block_prefix( fa_fn16( w ), lds4, &total );
    if (threadIdx.x == 0u) tile_fn[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024)
fasta_fn_scan_kernel(uint32_t* __restrict__ tile_fn, const uint32_t n_tiles, FaInfo* __restrict__ info)
{
    __shared__ uint32_t part[16];
    const uint32_t tot = bs_scan_in_place( tile_fn, n_tiles, BS_IDENTITY, [](const uint32_t a, const uint32_t b) -> uint32_t { return bs_compose( a, b ); }, part );
    if (threadIdx.x == 0u) info->final_machine = (tot >> (3u * info->snap.machine)) & 7u;
}

// the lane's 16 bytes and the state in front of them
__device__ __forceinline__ uint32_t fa_lane_state(const uint8_t* __restrict__ text, const uint32_t n, const uint64_t at, const uint32_t* __restrict__ tile_fn,
                                                  const FaInfo* __restrict__ info, uint32_t* lds4, uint32_t w[4])
{
    uint32_t total;
    bs_load16( text, n, at, FA_PAD, w );
    const uint32_t ex = bs_block_prefix( fa_fn16( w ), lds4, &total );
    const uint32_t entry = (tile_fn[blockIdx.x] >> (3u * info->snap.machine)) & 7u;
    return (ex >> (3u * entry)) & 7u;
}

// ---- the counts of every tile ----
__global__ void __launch_bounds__(256)
fasta_count_kernel(const uint8_t* __restrict__ text, const uint32_t n, const uint32_t* __restrict__ tile_fn, FaInfo* __restrict__ info, FaSum* __restrict__ tile_sum)
{
    __shared__ uint32_t lds4[4];
    __shared__ FaSum part[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t at = (uint64_t)blockIdx.x * BS_TILE + threadIdx.x * 16u;
    uint32_t w[4];
    uint32_t s = fa_lane_state( text, n, at, tile_fn, info, lds4, w );
    FaSum v = fa_nothing();
#pragma unroll
    for (uint32_t k = 0u; k < 16u; ++k)
    {
        const uint32_t c = bs_byte( w, k );
        if (at + k < n)
        {
            const uint32_t ev = fa_event( s, c );
            if (ev == FA_EV_SYMBOL)
            {
                const bool amb = fa_is_amb( c );
                ++v.sym;
                v.amb  += amb ? 1u : 0u;
                v.hole += (amb && v.last != c) ? 1u : 0u;
                if (v.first == FA_NOTHING) v.first = c;
                v.last = c;
            }
            else if (ev == FA_EV_START)
            {
                ++v.seq;
                if (v.first == FA_NOTHING) v.first = FA_RESET;
                v.last = FA_RESET;
            }
            else if (ev == FA_EV_NAME) ++v.name;
            else if (ev == FA_EV_END) info->end_off = (uint32_t)(at + k);           // END absorbs: one byte of the whole input does this
        }
        s = fa_next( s, c );
    }
    for (uint32_t o = 1u; o < 64u; o <<= 1) v = fa_combine( v, fa_shfl_down( v, o ) );      // lane 0: lanes 0 .. 63 in order (what other lanes hold is not used)
    if (lane == 0u) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0u) tile_sum[blockIdx.x] = fa_combine( fa_combine( part[0], part[1] ), fa_combine( part[2], part[3] ) );
}

// ---- ONE workgroup: tile_sum[t] = the counts of everything before tile t; the chunk's totals and the summary ----
__global__ void __launch_bounds__(1024)
fasta_sum_scan_kernel(FaSum* __restrict__ tile_sum, const uint32_t n_tiles, const uint32_t n, FaInfo* __restrict__ info, nvbio_fasta_summary* __restrict__ summary)
{
    __shared__ FaSum part[16];
    const FaSum tot = bs_scan_in_place( tile_sum, n_tiles, fa_nothing(), [](const FaSum a, const FaSum b) -> FaSum { return fa_combine( a, b ); }, part );
    if (threadIdx.x != 0u) return;
    const FaSum t = fa_combine( fa_before( info ), tot );
    const uint32_t fin = info->final_machine;
    uint32_t status = 0u;
    if (fin == NVBIO_FASTA_ID || fin == NVBIO_FASTA_REST) status |= NVBIO_FASTA_STATUS_INCOMPLETE;
    if (fin == NVBIO_FASTA_END) status |= NVBIO_FASTA_STATUS_END_BYTE;
    if ((uint64_t)info->snap.n_symbols + t.sym >= (1ull << 32) || (uint64_t)info->snap.n_name_bytes + t.name >= (1ull << 32))
    {
        status |= NVBIO_FASTA_STATUS_OVERFLOW_32;
        info->overflow = 1u;
    }
    info->total = t;
    *summary = nvbio_fasta_summary{ t.sym, t.seq, t.amb, t.hole, t.name,
                                    fin == NVBIO_FASTA_END ? (info->snap.machine == NVBIO_FASTA_END ? 0u : info->end_off) : n, fin, status };
}

// ---- encode ----
__global__ void __launch_bounds__(256)
fasta_zero_kernel(FaInfo* __restrict__ info, uint32_t* __restrict__ text2, const uint64_t capacity_words)
{
    if (blockIdx.x == 0u && threadIdx.x < 4u) info->freq[threadIdx.x] = 0u;
    if (info->overflow || text2 == nullptr) return;
    const uint64_t from = ((uint64_t)info->snap.n_symbols + 15u) >> 4, used = ((uint64_t)info->snap.n_symbols + info->total.sym + 15u) >> 4;
    const uint64_t to = used < capacity_words ? used : capacity_words;
    for (uint64_t i = from + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < to; i += (uint64_t)gridDim.x * 256u) text2[i] = 0u;
}

__global__ void __launch_bounds__(256)
fasta_emit_kernel(const uint8_t* __restrict__ text, const uint32_t n, const uint32_t* __restrict__ tile_fn, const FaSum* __restrict__ tile_sum,
                  FaInfo* __restrict__ info, uint32_t* __restrict__ text2, const uint64_t capacity_words, uint32_t* __restrict__ seq_offset,
                  uint32_t* __restrict__ name_index, const uint32_t max_seqs, uint8_t* __restrict__ names, const uint64_t names_capacity,
                  uint32_t* __restrict__ hole_offset, uint32_t* __restrict__ hole_rank, uint8_t* __restrict__ hole_amb, const uint32_t max_holes,
                  uint32_t* __restrict__ status)
{
    __shared__ uint32_t lds4[4], words[264];
    __shared__ uint64_t cnt4[4];
    __shared__ __attribute__((aligned(16))) uint8_t raw[BS_TILE], fresh[BS_TILE], code[BS_TILE];
    if (info->overflow) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t at = (uint64_t)blockIdx.x * BS_TILE + tid * 16u;
    uint32_t w[4];
    const uint32_t s0 = fa_lane_state( text, n, at, tile_fn, info, lds4, w );
    const FaSum P = fa_combine( fa_before( info ), tile_sum[blockIdx.x] );
    const uint32_t base_sym = info->snap.n_symbols + P.sym, base_seq = info->snap.n_seqs + P.seq, base_hole = info->snap.n_holes + P.hole,
                   base_name = info->snap.n_name_bytes + P.name;
    const uint64_t base_amb = (uint64_t)info->snap.n_ambs + P.amb;
    bool full = false;                                                             // an item did not fit
    ((uint4*)fresh)[tid] = uint4{ 0u, 0u, 0u, 0u };

    // where this lane's symbols, name bytes and sequence starts go: three counts in one sum (each is 4096 at most)
    uint64_t mine = 0ull;
    {
        uint32_t s = s0;
#pragma unroll
        for (uint32_t k = 0u; k < 16u; ++k)
        {
            const uint32_t c = bs_byte( w, k );
            if (at + k < n)
            {
                const uint32_t ev = fa_event( s, c );
                mine += ev == FA_EV_SYMBOL ? 1ull : ev == FA_EV_NAME ? (1ull << 16) : ev == FA_EV_START ? (1ull << 32) : 0ull;
            }
            s = fa_next( s, c );
        }
    }
    uint64_t inc = mine;
    for (uint32_t o = 1u; o < 64u; o <<= 1) { const uint64_t t = __shfl_up( inc, o, 64 ); if (lane >= o) inc += t; }
    if (lane == 63u) cnt4[wave] = inc;
    __syncthreads();
    uint64_t before = inc - mine, tile_total = 0ull;
    for (uint32_t v = 0u; v < 4u; ++v) { const uint64_t t = cnt4[v]; if (v < wave) before += t; tile_total += t; }
    const uint32_t n_sym = (uint32_t)tile_total & 0xFFFFu;

    // stage the symbols in output order; names and the sequences' entries go straight out
    {
        uint32_t s = s0, isym = (uint32_t)before & 0xFFFFu, iname = (uint32_t)(before >> 16) & 0xFFFFu, iseq = (uint32_t)(before >> 32);
#pragma unroll
        for (uint32_t k = 0u; k < 16u; ++k)
        {
            const uint32_t c = bs_byte( w, k );
            if (at + k < n)
            {
                const uint32_t ev = fa_event( s, c );
                if (ev == FA_EV_SYMBOL) raw[isym++] = (uint8_t)c;
                else if (ev == FA_EV_NAME)
                {
                    const uint64_t q = (uint64_t)base_name + iname++;
                    if (names) { if (q < names_capacity) names[q] = (uint8_t)c; else full = true; }
                }
                else if (ev == FA_EV_START)
                {
                    const uint32_t q = base_seq + iseq++;
                    if (isym < n_sym) fresh[isym] = 1u;                            // the next symbol is its sequence's first
                    if (seq_offset) { if (q < max_seqs) seq_offset[q] = base_sym + isym; else full = true; }
                    if (name_index) { if (q < max_seqs) name_index[q] = base_name + iname; else full = true; }
                }
            }
            s = fa_next( s, c );
        }
    }
    __syncthreads();

    // staged symbols 16 tid .. 16 tid + 15: ambiguous ones and hole starts, from the staged neighbour
    const uint32_t i0 = tid * 16u, i1 = i0 + 16u < n_sym ? i0 + 16u : n_sym;
    uint32_t ambm = 0u, holem = 0u;
    for (uint32_t i = i0; i < i1; ++i)
    {
        const uint32_t c = raw[i];
        if (!fa_is_amb( c )) continue;
        const uint32_t prev = fresh[i] ? FA_RESET : i ? (uint32_t)raw[i - 1u] : P.last;
        ambm |= 1u << (i - i0);
        if (prev != c) holem |= 1u << (i - i0);
    }
    const uint32_t mine2 = (uint32_t)__popc( ambm ) | ((uint32_t)__popc( holem ) << 16);
    uint32_t inc2 = mine2;
    for (uint32_t o = 1u; o < 64u; o <<= 1) { const uint32_t t = __shfl_up( inc2, o, 64 ); if (lane >= o) inc2 += t; }
    if (lane == 63u) lds4[wave] = inc2;
    __syncthreads();
    uint32_t before2 = inc2 - mine2;
    for (uint32_t v = 0u; v < wave; ++v) before2 += lds4[v];

    uint64_t rank = base_amb + (before2 & 0xFFFFu);                                // of this lane's next ambiguous symbol, in the whole input
    uint32_t h = base_hole + (before2 >> 16);
    uint64_t x = ambm ? fa_lcg_jump( fa_lcg_seed( info->snap.seed ), rank + 1u ) : 0ull;
    uint64_t f4 = 0ull;                                                            // the four frequencies, 16 bits each
    for (uint32_t i = i0; i < i1; ++i)
    {
        const uint32_t c = raw[i];
        uint32_t sc;
        if ((ambm >> (i - i0)) & 1u)
        {
            sc = (uint32_t)(x >> 46);
            if ((holem >> (i - i0)) & 1u)
            {
                if (hole_offset) { if (h < max_holes) hole_offset[h] = base_sym + i; else full = true; }
                if (hole_rank)   { if (h < max_holes) hole_rank[h] = (uint32_t)rank; else full = true; }
                if (hole_amb)    { if (h < max_holes) hole_amb[h] = (uint8_t)c; else full = true; }
                ++h;
            }
            ++rank;
            x = fa_lcg_step( x );
        }
        else sc = fa_code( c );
        code[i] = (uint8_t)sc;
        f4 += 1ull << (16u * sc);
    }
    for (uint32_t o = 32u; o; o >>= 1) f4 += __shfl_xor( f4, o, 64 );              // 4096 a tile at most: the fields do not carry
    if (lane == 0u)
        for (uint32_t j = 0u; j < 4u; ++j)
            if ((f4 >> (16u * j)) & 0xFFFFull) atomicAdd( &info->freq[j], (uint32_t)((f4 >> (16u * j)) & 0xFFFFull) );
    __syncthreads();

    // words: symbols [g0, g1) of the text are this tile's.  words[] holds them from the 16-byte boundary at or before the first on
    if (text2 && n_sym)
    {
        const uint64_t g0 = base_sym, g1 = g0 + n_sym;
        const uint32_t w0 = (uint32_t)(g0 >> 4), w1 = (uint32_t)((g1 - 1u) >> 4), wa = w0 & ~3u;
        for (uint32_t wd = wa + tid; wd <= w1; wd += 256u)
        {
            uint32_t word = 0u;
#pragma unroll
            for (uint32_t t = 0u; t < 16u; ++t)
            {
                const uint64_t g = (uint64_t)wd * 16u + t;
                if (g >= g0 && g < g1) word |= (uint32_t)code[g - g0] << (30u - 2u * t);
            }
            words[wd - wa] = word;
        }
        __syncthreads();
        const uint32_t groups = ((w1 - wa) >> 2) + 1u;
        for (uint32_t q = tid; q < groups; q += 256u)
        {
            const uint64_t W = (uint64_t)wa + 4u * q;
            if (W * 16u >= g0 && (W + 4u) * 16u <= g1 && W + 4u <= capacity_words)
                *(uint4*)(text2 + W) = uint4{ words[4u * q], words[4u * q + 1u], words[4u * q + 2u], words[4u * q + 3u] };
            else
                for (uint32_t j = 0u; j < 4u; ++j)
                {
                    const uint64_t wd = W + j;
                    if (wd < w0 || wd > w1) continue;
                    if (wd >= capacity_words) { full = true; continue; }
                    if (wd * 16u >= g0 && (wd + 1u) * 16u <= g1) text2[wd] = words[4u * q + j];
                    else atomicOr( &text2[wd], words[4u * q + j] );               // shared with the tile, or the chunk, on that side
                }
        }
    }
    if (full) atomicOr( status, NVBIO_FASTA_STATUS_CAPACITY );
}

__global__ void fasta_advance_kernel(const FaInfo* __restrict__ info, nvbio_fasta_state* __restrict__ state, uint32_t* __restrict__ status)
{
    if (info->overflow) { atomicOr( status, NVBIO_FASTA_STATUS_OVERFLOW_32 ); return; }
    nvbio_fasta_state s = info->snap;
    const FaSum t = info->total;
    s.machine = info->final_machine;
    s.n_symbols += t.sym; s.n_seqs += t.seq; s.n_ambs += t.amb; s.n_holes += t.hole; s.n_name_bytes += t.name;
    s.last_symbol = t.last;
    for (uint32_t j = 0u; j < 4u; ++j) s.freq[j] += info->freq[j];
    *state = s;
}

// ---- finish ----
__device__ __forceinline__ uint32_t fa_lower_bound(const uint32_t* __restrict__ a, uint32_t n, const uint32_t key)
{
    uint32_t lo = 0u;
    while (n) { const uint32_t half = n >> 1; if (a[lo + half] < key) { lo += half + 1u; n -= half + 1u; } else n = half; }
    return lo;
}

__global__ void __launch_bounds__(256)
fasta_finish_kernel(nvbio_fasta_state* __restrict__ state, uint32_t* __restrict__ seq_offset, uint32_t* __restrict__ name_index, const uint32_t max_seqs,
                    const uint32_t* __restrict__ hole_offset, const uint32_t* __restrict__ hole_rank, const uint32_t max_holes, uint32_t* __restrict__ hole_len,
                    uint32_t* __restrict__ seq_n_ambs)
{
    const uint32_t n_seqs = state->n_seqs, n_holes = state->n_holes, n_symbols = state->n_symbols, n_ambs = state->n_ambs, n_names = state->n_name_bytes;
    const uint32_t seqs = n_seqs < max_seqs ? n_seqs : max_seqs, holes = n_holes < max_holes ? n_holes : max_holes;
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    uint32_t longest = 0u;
    for (uint32_t s = id; s < seqs; s += step)
    {
        const bool last = s + 1u == n_seqs;
        if (name_index) { const uint32_t len = (last ? n_names : name_index[s + 1u]) - name_index[s]; longest = len > longest ? len : longest; }
        if (seq_n_ambs && seq_offset)
        {
            const uint32_t b = seq_offset[s], e = last ? n_symbols : seq_offset[s + 1u];
            seq_n_ambs[s] = hole_offset ? fa_lower_bound( hole_offset, holes, e ) - fa_lower_bound( hole_offset, holes, b ) : 0u;
        }
    }
    if (longest) atomicMax( &state->max_name_len, longest );
    if (hole_len && hole_rank)
        for (uint32_t h = id; h < holes; h += step) hole_len[h] = (h + 1u < holes ? hole_rank[h + 1u] : n_ambs) - hole_rank[h];
    if (id == 0u && n_seqs <= max_seqs)
    {
        if (seq_offset) seq_offset[n_seqs] = n_symbols;
        if (name_index) name_index[n_seqs] = n_names;
    }
}

// ---- the temp of both calls, laid out once ----
struct FaTemp
{
    FaInfo*   info;
    uint32_t* tile_fn;
    FaSum*    tile_sum;
    uint32_t  n_tiles;
    uint64_t  bytes;
};

static void fasta_temp(const uint64_t text_bytes, uint8_t* base, FaTemp* t)
{
    t->n_tiles = (uint32_t)((text_bytes + BS_TILE - 1u) / BS_TILE);
    ScratchLayout l( base );
    t->info     = l.take<FaInfo>( 1u );
    t->tile_fn  = l.take<uint32_t>( t->n_tiles );
    t->tile_sum = l.take<FaSum>( t->n_tiles );
    t->bytes    = l.bytes();
}

static nvbio_status fasta_refuse_4gib(const uint64_t text_bytes)
{
    if (text_bytes < (1ull << 32)) return NVBIO_OK;
    set_error( "fasta: a text of %llu bytes: offsets into the text are 32-bit, feed chunks below 4 GiB", (unsigned long long)text_bytes );
    return NVBIO_ERR_UNSUPPORTED;
}

// the checks of both calls that need no device
static nvbio_status fasta_check(const uint8_t* text_dev, const uint64_t text_bytes, const void* temp_dev, const uint64_t temp_bytes, FaTemp* t)
{
    NVB_CHECK( fasta_refuse_4gib( text_bytes ) );
    NVB_REQUIRE( text_bytes == 0u || text_dev != nullptr, "text_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)text_dev & 15u) == 0u, "text_dev must be 16-byte aligned" );
    NVB_REQUIRE( temp_dev != nullptr, "temp_dev is NULL" );
    uint8_t* base = (uint8_t*)(((uintptr_t)temp_dev + 255u) & ~(uintptr_t)255u);
    fasta_temp( text_bytes, base, t );
    NVB_REQUIRE( temp_bytes >= (uint64_t)(base - (uint8_t*)temp_dev) + ScratchLayout::round( t->bytes - 256u ), "temp_bytes too small (nvbio_fasta_temp_bytes)" );
    return NVBIO_OK;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

nvbio_status nvbio_fasta_state_init(int device, nvbio_fasta_state* state_dev, uint32_t seed, void* stream)
{
    NVB_REQUIRE( state_dev != nullptr, "state_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    return NVB_LAUNCH( fasta_state_init_kernel, dim3(1), dim3(1), (hipStream_t)stream, state_dev, seed );
}

nvbio_status nvbio_fasta_temp_bytes(uint64_t text_bytes, uint64_t* bytes)
{
    NVB_REQUIRE( bytes != nullptr, "bytes is NULL" );
    NVB_CHECK( fasta_refuse_4gib( text_bytes ) );
    FaTemp t; fasta_temp( text_bytes, nullptr, &t );
    *bytes = t.bytes;
    return NVBIO_OK;
}

nvbio_status nvbio_fasta_scan(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fasta_state* state_dev,
                              nvbio_fasta_summary* summary_dev, void* temp_dev, uint64_t temp_bytes, void* stream)
{
    FaTemp t; NVB_CHECK( fasta_check( text_dev, text_bytes, temp_dev, temp_bytes, &t ) );
    NVB_REQUIRE( state_dev != nullptr && summary_dev != nullptr, "state_dev or summary_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)text_bytes;
    NVB_CHECK( NVB_LAUNCH( fasta_init_kernel, dim3(1), dim3(1), s, t.info, state_dev ) );
    if (t.n_tiles) NVB_CHECK( NVB_LAUNCH( fasta_tile_fn_kernel, dim3(t.n_tiles), dim3(256), s, text_dev, n, t.tile_fn ) );
    NVB_CHECK( NVB_LAUNCH( fasta_fn_scan_kernel, dim3(1), dim3(1024), s, t.tile_fn, t.n_tiles, t.info ) );
    if (t.n_tiles) NVB_CHECK( NVB_LAUNCH( fasta_count_kernel, dim3(t.n_tiles), dim3(256), s, text_dev, n, t.tile_fn, t.info, t.tile_sum ) );
    return NVB_LAUNCH( fasta_sum_scan_kernel, dim3(1), dim3(1024), s, t.tile_sum, t.n_tiles, n, t.info, summary_dev );
}

nvbio_status nvbio_fasta_encode(int device, const uint8_t* text_dev, uint64_t text_bytes, void* temp_dev, uint64_t temp_bytes,
                                nvbio_fasta_state* state_dev, uint32_t* text2_dev, uint64_t text2_capacity_words, uint32_t* seq_offset_dev,
                                uint32_t* name_index_dev, uint32_t max_seqs, uint8_t* names_dev, uint64_t names_capacity, uint32_t* hole_offset_dev,
                                uint32_t* hole_rank_dev, uint8_t* hole_amb_dev, uint32_t max_holes, uint32_t* status_dev, void* stream)
{
    FaTemp t; NVB_CHECK( fasta_check( text_dev, text_bytes, temp_dev, temp_bytes, &t ) );
    NVB_REQUIRE( state_dev != nullptr && status_dev != nullptr, "state_dev or status_dev is NULL" );
    NVB_REQUIRE( ((uintptr_t)text2_dev & 15u) == 0u, "text2_dev must be 16-byte aligned" );
    NVB_REQUIRE( text2_capacity_words <= (1ull << 28), "text2_capacity_words must not exceed 2^28 (2^32 symbols)" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    NVB_CHECK( NVB_LAUNCH( fasta_zero_kernel, dim3(grid_for( text_bytes / 16u + 2u )), dim3(256), s, t.info, text2_dev, text2_capacity_words ) );
    if (t.n_tiles)
        NVB_CHECK( NVB_LAUNCH( fasta_emit_kernel, dim3(t.n_tiles), dim3(256), s, text_dev, (uint32_t)text_bytes, t.tile_fn, t.tile_sum, t.info, text2_dev,
                               text2_capacity_words, seq_offset_dev, name_index_dev, max_seqs, names_dev, names_capacity, hole_offset_dev, hole_rank_dev,
                               hole_amb_dev, max_holes, status_dev ) );
    return NVB_LAUNCH( fasta_advance_kernel, dim3(1), dim3(1), s, t.info, state_dev, status_dev );
}

nvbio_status nvbio_fasta_finish(int device, nvbio_fasta_state* state_dev, uint32_t* seq_offset_dev, uint32_t* name_index_dev, uint32_t max_seqs,
                                const uint32_t* hole_offset_dev, const uint32_t* hole_rank_dev, uint32_t max_holes, uint32_t* hole_len_dev,
                                uint32_t* seq_n_ambs_dev, void* stream)
{
    NVB_REQUIRE( state_dev != nullptr, "state_dev is NULL" );
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    const uint64_t most = max_seqs > max_holes ? max_seqs : max_holes;
    return NVB_LAUNCH( fasta_finish_kernel, dim3(grid_for( most, 256u, 4096u )), dim3(256), (hipStream_t)stream, state_dev, seq_offset_dev, name_index_dev,
                       max_seqs, hole_offset_dev, hole_rank_dev, max_holes, hole_len_dev, seq_n_ambs_dev );
}

} // extern "C"
