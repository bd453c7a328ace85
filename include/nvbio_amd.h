/* nvbio_amd.h -- C ABI of the MI355X-native seed-and-extend core.
 *
 * This is the drop-in boundary for the hot path of NVBIO / nvBowtie: FM-index
 * rank / match / locate over a 2-bit packed BWT and batched (banded and full-matrix)
 * Gotoh scoring.  The reference has no C ABI; its operator API for this path is three
 * template concepts.  Every entry point below names the reference
 * interface it stands in for (file:line relative to the reference tree); the C++
 * shim that plugs these calls back under the reference's own class names is in
 * nvbio-gpl_amd/host/, and INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - plain C types only; every `*_dev` / "device pointer" argument is a pointer into the
 *     HBM of the GPU the handle/stream lives on; the caller owns those buffers.
 *   - all entry points return an nvbio_status (0 = ok) and never throw; a message for the
 *     last failure on the calling thread is available from nvbio_amd_last_error().
 *   - work is enqueued on the caller's stream (a hipStream_t passed as void*; NULL = the
 *     default stream) and is asynchronous; nvbio_amd_stream_synchronize() (or the caller's
 *     own hipStreamSynchronize) waits for it.  Calls on one handle from several host
 *     threads are safe as long as each thread uses its own stream and output buffers.
 *   - scratch a call needs beyond the caller's buffers (job lists, boundary columns, scan temporaries) comes from device blocks the
 *     library allocates with hipMalloc and KEEPS, per (device, stream), for the next call on that stream: after the first calls at a
 *     given size no call allocates.  nvbio_amd_release_scratch() gives the idle blocks back (it synchronises their streams).
 *   - results are bit-identical to the reference's CPU path: SA ranges, SA rows and text
 *     positions as uint32, scores as int32, sinks as (text, pattern) uint32 pairs.
 */
#ifndef NVBIO_AMD_H
#define NVBIO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVBIO_AMD_VERSION 100   /* 0.1.0 */

typedef enum
{
    NVBIO_OK              = 0,
    NVBIO_ERR_INVALID     = 1,  /* bad argument (null pointer, unsupported band/bits, ...)   */
    NVBIO_ERR_HIP         = 2,  /* a HIP runtime call failed                                   */
    NVBIO_ERR_NOMEM       = 3,  /* device or host allocation failed                            */
    NVBIO_ERR_UNSUPPORTED = 4,  /* valid in the reference but not built here                   */
    NVBIO_ERR_NO_DEVICE   = 5   /* no usable gfx950 device: the library has NO CPU fallback    */
} nvbio_status;

int         nvbio_amd_version(void);
const char* nvbio_amd_last_error(void);
/* number of visible HIP devices and the gcnArchName of one of them (e.g. "gfx950:sramecc+:xnack-") */
nvbio_status nvbio_amd_device_count(int* count);
nvbio_status nvbio_amd_device_arch(int device, char* name, uint32_t name_len);
nvbio_status nvbio_amd_stream_synchronize(int device, void* stream);
/* hipFree every scratch block that no call is using (see "Conventions"); each behind a synchronisation of the stream it served */
nvbio_status nvbio_amd_release_scratch(void);
/* check mode: every scratch block exact-size, guard-banded, filled with `fill`; set only between calls */
nvbio_status nvbio_amd_set_scratch_check(int enable, uint32_t fill_byte);
/* one text line per site seen since the last enable: "<tag> <blocks checked> <blocks damaged> <first bad sub-array> <first bad offset>"
 * (a test tool: with check mode on, each scratch block is a fresh hipMalloc with a 4 KiB guard band at each end, a layout leaves 256 bytes before
 * each sub-array and after the last, a caller's temp_dev is filled whole, so the *_temp_bytes queries grow: query after enabling.  When the block
 * goes out of use its bands and gaps are read back.  The first bad sub-array is the one that precedes the first damaged byte, -1 before the
 * first; the offset is in bytes from the block's first sub-array.  A clean site prints "- -" for both.) */
nvbio_status nvbio_amd_scratch_check_report(char* buf, uint64_t buf_len);

/* -------------------------------------------------------------------------------------------
 * pair of uint32, layout-compatible with the reference's uint2 (SA ranges, hits, sinks)
 * ------------------------------------------------------------------------------------------- */
typedef struct { uint32_t x, y; } nvbio_uint2;

/* -------------------------------------------------------------------------------------------
 * FM-index
 * ------------------------------------------------------------------------------------------- */

/* Storage-free view of an FM-index resident in HBM: the members of nvbio::fm_index
 * (nvbio/fmindex/fmindex.h:320-361) in the production layout of io::FMIndexDataDevice
 * (nvbio/io/fmindex/fmindex.h:75-177, :294-295):
 *   bwt_occ : 32-byte records; record k = 4 words of 2-bit big-endian BWT symbols [64k,64k+64)
 *             followed by 4 words occ{A,C,G,T} = counts in BWT[0,64k)   (fmindex_impl.cu:300-313)
 *   ssa     : ssa[j] = SA[sa_int j], ssa[0] = 0xFFFFFFFF                (ssa_inl.h:254-301,477-495)
 *             sa_int = 16 is the reference's production layout (SA_INT, io/fmindex/fmindex.h:86);
 *             indices built here may sample more densely (a power of two down to 1 = the full
 *             suffix array, 12 GB for 3 Gbp): positions returned by locate() do not depend on it
 *   L2      : L2[c] = number of symbols < c, L2[4] = length             (fmindex.h:335-336)       */
typedef struct
{
    uint32_t        length;          /* n: text symbols (the BWT holds n symbols, '$' is implicit)  */
    uint32_t        primary;         /* BWT-matrix row of '$'                                       */
    uint32_t        L2[5];
    const uint32_t* bwt_occ_dev;     /* device pointer, 32-byte aligned                             */
    uint64_t        bwt_occ_words;   /* = 2 * ceil4(ceil(n/16))                                     */
    const uint32_t* ssa_dev;         /* device pointer, may be NULL (match-only index)              */
    uint64_t        ssa_words;       /* = n/sa_int + 1                                              */
    uint32_t        sa_int;          /* SA sampling interval: power of two in [1,64]; 0 means 16    */
} nvbio_fm_index_view;

typedef struct nvbio_fm_index_s* nvbio_fm_index_t;     /* opaque handle */

/* Wrap an index that is already in HBM (the caller keeps ownership of bwt_occ/ssa, as with the
 * reference's storage-free views).  kmer_len > 0 additionally builds, on the GPU, a table with
 * the SA range of every kmer_len-mer (4^kmer_len x 8 bytes, owned by the handle) which match()
 * uses to replace its first kmer_len backward-search steps with one lookup; results are
 * identical with and without it.  kmer_len = 0 disables it; values up to 17 are accepted
 * (k = 12: 128 MiB, k = 14: 2 GiB, k = 16: 32 GiB, k = 17: 128 GiB -- sized for 288 GB of HBM).
 * A handle that also holds the full suffix array and the text (nvbio_fm_index_build with sa_int = 1) keeps the last TWO
 * levels of the table: level kmer_len - 1 as the table of match(), and level kmer_len as the table of the direct seed pass
 * (nvbio_fm_match_direct, nvbio_fm_match_seed_diagonals): the entry of a k-mer with ONE occurrence rewritten to that
 * occurrence's text position and the 15 text symbols to its left, that of a k-mer with 2..7 occurrences pointing to a
 * 32/64-byte group with the same for each of them -- a 22-mer seed of a 3 Gbp genome is then matched AND located by the
 * table gather alone (texts up to 3.22 G symbols; longer ones keep positions without the context).
 * Replaces: constructing nvbio::fm_index / io::FMIndexDataDevice (nvbio/io/fmindex/fmindex_impl.cu:740-816). */
nvbio_status nvbio_fm_index_create(const nvbio_fm_index_view* view, int device, uint32_t kmer_len,
                                   void* stream, nvbio_fm_index_t* out);

/* Build the whole index on the GPU from a 2-bit big-endian packed text in HBM (layout of
 * io::SequenceData<DNA>, nvbio/io/sequence/sequence_traits.h:32-38): suffix sort, BWT, occ,
 * interleave, SSA.  All arrays are owned by the handle.  Replaces, for synthetic / benchmark
 * references, the offline nvBWT + FMIndexDataHost::load path (nvBWT/nvBWT.cu,
 * nvbio/io/fmindex/fmindex_impl.cu:111-331) and SSA_index_multiple's builder (ssa_inl.h:273-470).
 * Texts with repeats longer than options->max_lcp symbols are rejected with NVBIO_ERR_UNSUPPORTED
 * rather than sorted slowly. */
typedef struct
{
    uint32_t kmer_len;   /* k of the k-mer SA-range table, 0..17 (0 = none)                                  */
    uint32_t sa_int;     /* SA sampling interval, power of two in [1,64]; 0 = 16 (the reference's SA_INT)     */
    uint32_t max_lcp;    /* give up on texts with repeats longer than this many symbols; 0 = 4096            */
    uint32_t verify;     /* 1: also keep the inverse suffix array (4(n+1) bytes) and a copy of the text, so that
                            match() can finish a search whose range has collapsed to ONE row by comparing the
                            rest of the pattern with the text at SA[row] and jumping to ISA[position] (3 gathers
                            instead of one per remaining symbol).  Requires sa_int = 1.  Results are identical. */
    uint32_t table_flags;     /* NVBIO_FM_TABLE_*: which form of the k-mer tables a direct-capable handle keeps (A/B measurements and
                                 tests; results are identical with every combination)                                              */
    uint32_t bucket_symbols;  /* suffix sort: 0 = choose the number of prefix symbols used for bucketing from the text length;
                                 1 + v forces v in 0..4 (tests run the bucketed path on small texts this way)                      */
} nvbio_fm_build_options;

enum
{
    NVBIO_FM_TABLE_NO_DIRECT  = 1,  /* keep the plain SA-range table only, even if the handle holds the full SA and the text      */
    NVBIO_FM_TABLE_NO_CONTEXT = 2,  /* direct table, format 1: one-row entries hold the position only (the rest of a seed is then
                                       verified with a gather from the text)                                                      */
    NVBIO_FM_TABLE_NO_GROUPS  = 4,  /* no groups for k-mers with 2..7 occurrences (they keep their SA range and take rank steps)  */
    NVBIO_FM_TABLE_CANONICAL_WIDE = 16, /* NVBIO_FM_TABLE_CANONICAL with 16-byte entries: a k-mer with TWO occurrences (of either orientation) has
                                       both rows in its entry, so that only k-mers with three or more take the second gather (1.07 instead
                                       of 1.25 sectors per seed window on a 3 Gbp text; 128 GiB at k = 17)                         */
    NVBIO_FM_TABLE_NO_TEXT_PLANES = 32, /* a handle that keeps the text does not also keep it as bit planes (nvbio_fm_index_text_planes: none)  */
    NVBIO_FM_TABLE_NO_SEED_LOCUS = 64,  /* a handle with the canonical table does not build the seed locus lines (nvbio_fm_index_seed_locus: none) */
    NVBIO_FM_TABLE_CANONICAL  = 8   /* instead of the direct table: ONE table for a k-mer and its reverse complement (kmer_len odd; 64 GiB at
                                       k = 17 where the direct table takes 128), serving nvbio_fm_match_seed_diagonals_both; the plain table of
                                       (kmer_len - 1)-mers is kept for match().  Needs sa_int = 1.                                */
};

nvbio_status nvbio_fm_index_build(const uint32_t* text2_dev, uint32_t length, int device,
                                  const nvbio_fm_build_options* options /* NULL = defaults */,
                                  void* stream, nvbio_fm_index_t* out);

/* Load an index from the reference's on-disk files (written by nvBWT, nvBWT/nvBWT.cu:303-342; read by
 * io::FMIndexDataHost::load, nvbio/io/fmindex/fmindex_impl.cu:111-252,333-...):
 *   <bwt_path>  uint32 primary; uint32 cumulative symbol counts[4] (last = n); packed 2-bit BWT words
 *   <sa_path>   uint32 primary; uint32 counts[4]; uint32 SA_INT; uint32 n; ssa[1..]   (optional, may be NULL)
 * The occurrence table is rebuilt and interleaved on the GPU (the reference does it on the host,
 * fmindex_impl.cu:254-331).  All arrays are owned by the handle. */
nvbio_status nvbio_fm_index_load(const char* bwt_path, const char* sa_path, int device, uint32_t kmer_len,
                                 void* stream, nvbio_fm_index_t* out);
/* Write the index in those formats (the role of nvBWT for indices built by nvbio_fm_index_build);
 * sa_path may be NULL.  The reference's reader accepts .sa files with SA_INT = 16 only. */
nvbio_status nvbio_fm_index_save(nvbio_fm_index_t index, const char* bwt_path, const char* sa_path, void* stream);

nvbio_status nvbio_fm_index_destroy(nvbio_fm_index_t index);
nvbio_status nvbio_fm_index_get_view(nvbio_fm_index_t index, nvbio_fm_index_view* view);
/* copy the index arrays into caller buffers in HBM (either may be NULL); sizes from get_view */
nvbio_status nvbio_fm_index_export(nvbio_fm_index_t index, uint32_t* bwt_occ_out_dev, uint32_t* ssa_out_dev, void* stream);
/* bytes of HBM owned by the handle (k-mer table, and the index arrays if it was built here) */
nvbio_status nvbio_fm_index_device_bytes(nvbio_fm_index_t index, uint64_t* bytes);

/* The text as bit planes, the constant input of the band-31 end-to-end passes (nvbio_alignment_batch::text_planes_dev).
 * A unit is 16 bytes, (lo64, hi64) of 64 consecutive symbols: bit j of lo64 / hi64 = the low / high bit of symbol 64 u + j.
 * Line L (128 bytes) holds units 4 L .. 4 L + 7, i.e. symbols 256 L .. 256 L + 511 -- consecutive lines overlap by half, so
 * the up to 197 symbols a job looks at, from any symbol tb on, lie in the ONE line tb >> 8.  ((length + 255) >> 8) + 1 lines
 * (twice the packed text: 1.5 GB at 3 Gbp); every bit at or beyond `length` is zero.
 * nvbio_text_planes_build: one streaming pass over the 2-bit big-endian packed text ((length + 15) / 16 words are read) into
 * the caller's buffer of nvbio_text_planes_bytes bytes, which must be 128-byte aligned (NVBIO_ERR_INVALID otherwise). */
nvbio_status nvbio_text_planes_bytes(uint32_t length, uint64_t* bytes);
nvbio_status nvbio_text_planes_build(int device, const uint32_t* text2_dev, uint32_t length, void* planes_dev, void* stream);
/* The planes a handle keeps: one that keeps the text (nvbio_fm_index_build with sa_int = 1) builds them from its copy unless
 * NVBIO_FM_TABLE_NO_TEXT_PLANES is set, and counts them in nvbio_fm_index_device_bytes.  *planes_dev = NULL (and *length = 0)
 * where there are none.  Like the handle itself they describe the text as it was when the index was built. */
nvbio_status nvbio_fm_index_text_planes(nvbio_fm_index_t index, const void** planes_dev, uint32_t* length);

/* The seed locus lines of the two-strand seed pass (nvbio_fm_match_seed_diagonals_both): the text's bit planes beside a uniqueness
 * plane u for ONE seed length, so that a read placed by its first seed settles its other seeds from one 128-byte line.
 * A unit is 24 bytes, (lo64, hi64, u64) of 64 consecutive symbols: lo64 / hi64 as in the text planes, bit j of u64 = u[64 unit + j].
 * Line L (128 bytes) holds units 2 L .. 2 L + 4, i.e. symbols 128 L .. 128 L + 319, then 8 zero bytes: a read of up to 193 symbols
 * that begins at symbol P0 lies in the ONE line P0 >> 7.  (length >> 7) + 1 lines (3.0 GB at 3 Gbp); every bit at or beyond
 * `length` is zero.  u[x] = 1 only if text[x, x + seed_len) occurs exactly once in the text and its reverse complement nowhere --
 * precisely: iff the canonical table answers that window with the forward hit x alone and its reverse complement with the
 * reverse-strand hit x alone, neither through a k-mer with more than 8 occurrences; u is 0 in the last seed_len - 1 positions.
 * nvbio_seed_locus_build: one gather pass over the text positions into the caller's buffer of nvbio_seed_locus_bytes bytes, which
 * must be 128-byte aligned (NVBIO_ERR_INVALID otherwise); the handle needs the canonical table and the text
 * (NVBIO_FM_TABLE_CANONICAL, sa_int = 1), seed_len lies in [kmer_len, kmer_len + 7].
 * The lines a handle keeps: such a handle builds them for seed_len = 22 where kmer_len <= 22 <= kmer_len + 7, unless
 * NVBIO_FM_TABLE_NO_SEED_LOCUS is set, and counts them in nvbio_fm_index_device_bytes.  nvbio_fm_index_seed_locus hands them out
 * (*lines_dev = NULL and *seed_len = 0 where there are none); nvbio_fm_index_build_seed_locus builds them, or rebuilds them for
 * another seed length (it synchronises the stream; no seed pass of the handle may be in flight). */
nvbio_status nvbio_seed_locus_bytes(uint32_t length, uint64_t* bytes);
nvbio_status nvbio_seed_locus_build(nvbio_fm_index_t index, uint32_t seed_len, void* lines_dev, void* stream);
nvbio_status nvbio_fm_index_seed_locus(nvbio_fm_index_t index, const void** lines_dev, uint32_t* seed_len);
nvbio_status nvbio_fm_index_build_seed_locus(nvbio_fm_index_t index, uint32_t seed_len, void* stream);

/* A set of query strings in HBM: the string-set concept FMIndexFilter::rank consumes
 * (nvbio/fmindex/filter.h:52-231) flattened to arrays.
 *   symbols      packed big-endian words (symbol_bits 2 or 4: PackedStream<..,true>,
 *                nvbio/basic/packedstream_inl.h:33-75; 4-bit = io::SequenceData<DNA_N>) or one
 *                symbol per byte (symbol_bits 8).  Symbols > 3 are 'N'.
 *   offsets      if offsets_are_ranges: n+1 entries, string i = [offsets[i], offsets[i+1])
 *                else if non-NULL: n entries, string i = [offsets[i], offsets[i]+fixed_len)
 *                else: string i = [i*stride, i*stride + fixed_len)                             */
typedef struct
{
    const void*     symbols_dev;
    uint32_t        symbol_bits;
    const uint32_t* offsets_dev;
    uint32_t        offsets_are_ranges;
    uint32_t        fixed_len;
    uint32_t        stride;
    uint32_t        n;
    /* seed enumeration (uniform_seeds_functor, nvbio/strings/seeds.h; nvBowtie mapping_inl.h:485-556):
     * if seeds_per_string > 0 the set is the seeds of a set of n / seeds_per_string strings: query i is
     * seed j = i % seeds_per_string of string r = i / seeds_per_string,
     *   [ base(r) + j*seed_interval, + fixed_len ),  base(r) = offsets_dev ? offsets_dev[r] : r*stride   */
    uint32_t        seeds_per_string;
    uint32_t        seed_interval;
    /* ragged seed sets (reads of different lengths, each seeded at its own interval: nvBowtie computes both per read,
     * mapping_inl.h:507-529, `read_len = range.y - range.x`, `seed_freq( read_len )`): seed_intervals_dev[r] = the seed interval of
     * string r (n / seeds_per_string entries), or NULL.  With it offsets_dev holds n_strings + 1 entries (string r =
     * [offsets[r], offsets[r+1]) ), seeds_per_string is the LARGEST number of seeds of a string -- the stride of seed ids, seed id =
     * r * seeds_per_string + j -- and seed j of string r exists iff j * interval_r + fixed_len <= its length; a seed id without a seed
     * matches nothing (the empty range (1, 0)).  seed_interval is ignored. */
    const uint32_t* seed_intervals_dev;
} nvbio_string_set;

enum
{
    NVBIO_FM_SCAN_FORWARD = 1,   /* consume symbols 0..len-1 (match_reverse, fmindex_inl.h:247-278; nvBowtie
                                    match_range, mapping_inl.h:73-86); default is len-1..0 (match, :181-239) */
    NVBIO_FM_COMPLEMENT   = 2,   /* search the complement (c < 4 ? 3-c : c), as nvBowtie's rc seeds
                                    (mapping_inl.h:264-279)                                                   */
    NVBIO_FM_NO_KMER_TABLE = 4,  /* step every symbol through rank() even if the handle has a table         */
    NVBIO_FM_NO_VERIFY     = 8,  /* never take the SA/ISA verification shortcut even if the handle has it   */
    NVBIO_FM_COUNT_SECTORS = 16, /* nvbio_fm_match_seed_diagonals only: an accounting launch (see there)        */
    NVBIO_FM_NO_PIPELINE   = 32  /* nvbio_fm_match_seed_diagonals only: the plain kernel, one tile at a time,
                                    also where the software-pipelined one applies (A/B; same results)         */
};

/* ranges_dev[i] = SA range (inclusive; empty iff x > y) of query i: nvbio::match / match_reverse
 * (nvbio/fmindex/fmindex_inl.h:181-278), including the N rule (-> (1,0)) and the reference's
 * early-exit values for patterns that stop matching.
 * blocks_dev (optional): number of distinct 32-byte bwt_occ records the reference's algorithm
 * touches for query i (the algorithmic-traffic unit of SURVEY.md 8d); requires NO_KMER_TABLE. */
nvbio_status nvbio_fm_match(nvbio_fm_index_t index, const nvbio_string_set* queries, uint32_t flags,
                            nvbio_uint2* ranges_dev, uint32_t* blocks_dev, void* stream);

/* rank(fmi, k, c) for n (row, symbol) pairs: nvbio/fmindex/fmindex_inl.h:27-47 */
nvbio_status nvbio_fm_rank(nvbio_fm_index_t index, const uint32_t* rows_dev, const uint8_t* syms_dev, uint32_t n,
                           uint32_t* out_dev, void* stream);
/* rank4(fmi, k): counts of all four symbols, fmindex_inl.h:96-123 (out_dev: 4 words per row) */
nvbio_status nvbio_fm_rank4(nvbio_fm_index_t index, const uint32_t* rows_dev, uint32_t n,
                            uint32_t* out_dev, void* stream);

/* The GENERIC rank dictionary of the reference (nvbio/fmindex/rank_dictionary.h; dispatch_rank over plain words,
 * rank_dictionary_inl.h:206-336): 2-bit big-endian text in 32- or 64-bit words (PackedStream<const uint32*|const uint64*,uint8,2,true>),
 * a separate occurrence table occ[4 k + c] = # c in text[0, k K) (build_occurrence_table<K>, :33-66), indices and counts of 32 or 64 bits
 * -- the layouts of the reference's own rank test (nvbio-test/rank_test.cu:83-227: uint32 / K = 64; uint64 / K = 128 with 64-bit indices),
 * and the one to use beyond 2^32 symbols.  (The production layout, 32-byte records of BWT + occ, is served by nvbio_fm_rank.)
 *   nvbio_rank_dictionary_occ_entries : entries (of index_bits each) the occurrence table needs = 4 ceil(length / K)
 *   nvbio_rank_dictionary_build       : fills occ_out_dev; counts[c] (host) = total occurrences of c; synchronizes
 *   nvbio_rank_dictionary_rank        : out[q] = rank( dict, idx[q], sym[q] ) = occurrences of sym[q] in text[0, idx[q]] (inclusive);
 *                                       idx = all ones (-1) gives 0 (:278-279); idx / out are index_bits wide
 *   nvbio_rank_dictionary_rank4       : out[4 q + c] = rank( dict, idx[q], c ) for the four symbols (rank4, :294-309)            */
typedef struct
{
    const void* text_dev;
    uint32_t    word_bits;     /* 32 or 64 */
    const void* occ_dev;       /* NULL for nvbio_rank_dictionary_build */
    uint32_t    index_bits;    /* 32 or 64 */
    uint32_t    K;             /* symbols per block: a power of two, a multiple of the symbols per word */
    uint64_t    length;        /* symbols */
} nvbio_rank_dictionary;
nvbio_status nvbio_rank_dictionary_occ_entries(const nvbio_rank_dictionary* dict, uint64_t* entries);
nvbio_status nvbio_rank_dictionary_build(int device, const nvbio_rank_dictionary* dict, void* occ_out_dev, uint64_t counts[4], void* stream);
nvbio_status nvbio_rank_dictionary_rank(int device, const nvbio_rank_dictionary* dict, const void* idx_dev, const uint8_t* syms_dev, uint32_t n,
                                        void* out_dev, void* stream);
nvbio_status nvbio_rank_dictionary_rank4(int device, const nvbio_rank_dictionary* dict, const void* idx_dev, uint32_t n, void* out_dev, void* stream);

/* out_dev[i] = basic_inv_psi(fmi, rows_dev[i]): one LF step, the row of the suffix one symbol to the
 * left (nvbio/fmindex/fmindex_inl.h:286-309); rows_dev == out_dev is allowed */
nvbio_status nvbio_fm_basic_inv_psi(nvbio_fm_index_t index, const uint32_t* rows_dev, uint32_t n,
                                    uint32_t* out_dev, void* stream);

/* pos_dev[i] = text position of SA row rows_dev[i]: nvbio::locate (fmindex_inl.h:360-394).
 * rows_dev == pos_dev is allowed (nvBowtie locates in place, locate_inl.h:113-138). */
nvbio_status nvbio_fm_locate(nvbio_fm_index_t index, const uint32_t* rows_dev, uint32_t n,
                             uint32_t* pos_dev, void* stream);
/* match() + locate() fused for the searches that end in a single text occurrence (the common case of a seed
 * pass: a 22-mer of a 3 Gbp genome).  As nvbio_fm_match, except that a search whose SA range has collapsed to
 * ONE row before the pattern is exhausted is finished on the text to the left of SA[row] instead of by one
 * rank step per remaining symbol: 2 dependent gathers instead of (remaining symbols + the later SA lookup).
 * For such a query  direct_dev[i] = 1  and  ranges_dev[i] = (pos, pos)  where pos is the TEXT POSITION of the
 * occurrence -- exactly locate(fmi, row) of the one row the reference's match() would end in -- or, if the rest
 * of the pattern does not match, direct_dev[i] = 0 and the empty range (1,0).  Every other query gets
 * direct_dev[i] = 0 and its SA range as from nvbio_fm_match.  Range sizes (and so nvbio_fm_filter_scan) are
 * unaffected; nvbio_fm_filter_locate_direct expands the mix into the same hits, in the same order, as
 * nvbio_fm_filter_locate does on the plain ranges.  Needs the handle to hold the full suffix array and the text
 * (nvbio_fm_index_build with sa_int = 1), else NVBIO_ERR_UNSUPPORTED. */
nvbio_status nvbio_fm_match_direct(nvbio_fm_index_t index, const nvbio_string_set* queries, uint32_t flags,
                                   nvbio_uint2* ranges_dev, uint8_t* direct_dev, void* stream);
/* *yes = 1 iff the handle can serve nvbio_fm_match_direct (it holds the full suffix array and the text) */
nvbio_status nvbio_fm_index_supports_direct(nvbio_fm_index_t index, int* yes);
nvbio_status nvbio_fm_filter_locate_direct(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev,
                                           const uint8_t* direct_dev, uint32_t n_queries, uint64_t begin, uint64_t end,
                                           nvbio_uint2* hits_dev, void* stream);

/* nvbio_fm_filter_locate[_direct] and nvbio_hits_to_diagonals (below) in one pass: the expansion writes each hit's
 * diagonal key (read << 34 | strand << 33 | diagonal + 1024) instead of the (position, query) pair; direct_dev may
 * be NULL (plain ranges).  keys_dev[h - begin] equals nvbio_hits_to_diagonals of the hit nvbio_fm_filter_locate writes.
 * query_ids_dev (optional): the seed id of query i when the ranges are a compacted subset of a seed set (the residual
 * list of nvbio_fm_match_seed_diagonals); NULL = query i is seed i.  Bit 31 of a query id flips `strand` for that query (seed ids are
 * below 2^31), so that the two residual lists of nvbio_fm_match_seed_diagonals_both can go through one call. */
nvbio_status nvbio_fm_filter_locate_diagonals(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev,
                                              const uint8_t* direct_dev, uint32_t n_queries, uint64_t begin, uint64_t end,
                                              uint32_t seeds_per_read, uint32_t seed_interval, uint32_t seed_len, uint32_t read_len,
                                              uint32_t strand, const uint32_t* query_ids_dev, uint64_t* keys_dev, void* stream);

/* Approximate matching by backtracking under the Hamming distance: nvbio::hamming_backtrack (nvbio/fmindex/backtrack.h:51-157),
 * the kernel of the reference's "approximate search" benchmark (nvbio-test/fmindex_test.cu:739-800; the building block of
 * nvBowtie's approximate seed mapper, mapping_inl.h:114-184).  The last seed_len symbols of every query are matched exactly, the
 * rest may differ from the text in up to `mismatches` positions.
 *   counts_dev[i]   = total number of occurrences (the reference benchmark's CountDelegate: sum of the reported range sizes)
 *   n_ranges_dev[i] = number of SA ranges the delegate receives (optional)
 *   ranges_dev      = (optional) the first max_ranges of them per query, [i * max_ranges + k], in the reference's order
 * The traversal uses the reference benchmark's 128-entry stack; a query that would overflow it makes the call return
 * NVBIO_ERR_UNSUPPORTED (the reference writes past its array there).  Synchronises the stream.
 * flags: by default a branch stops when it reaches the start of the pattern, as the reference documents.  The reference's code
 * does not (backtrack.h:110-116 falls through at l == 0): a branch arriving there with all mismatches used reports its range
 * twice, and one arriving with some left continues through the symbols that PRECEDE the query in its stream, every branch it
 * spawns there ending in a report.  NVBIO_BACKTRACK_REFERENCE_QUIRKS reproduces exactly that (queries must then not start at
 * symbol 0 of the stream; pinned against the reference's own code over PackedStream patterns, tests/golden/bt_golden.npz). */
enum { NVBIO_BACKTRACK_REFERENCE_QUIRKS = 1 };
nvbio_status nvbio_fm_hamming_backtrack(nvbio_fm_index_t index, const nvbio_string_set* queries, uint32_t seed_len, uint32_t mismatches, uint32_t flags,
                                        uint32_t* counts_dev, uint32_t* n_ranges_dev, nvbio_uint2* ranges_dev, uint32_t max_ranges, void* stream);

/* The whole seed pass of one strand, for handles that hold the full suffix array and the text: nvBowtie's
 * match_range over every seed (mapping_inl.h:73-86,193-282) followed, for every seed that ends on ONE SA row, by what
 * FMIndexFilter::rank's scan, FMIndexFilter::locate (filter_inl.h:193-252), hit_to_diagonal (examples/fmmap/fmmap.cu:92-117)
 * and the removal of adjacent duplicate diagonals would do with it: the hit's diagonal key goes straight to keys_dev
 * (as nvbio_fm_filter_locate_diagonals writes it), IN SEED ORDER; a key equal to the previous key of the same read is
 * dropped (consecutive seeds of a read that agree on the diagonal).  Seeds that end on several rows go to the residual list
 * (residual_ranges_dev[r], residual_ids_dev[r] = seed id, in arbitrary order) for nvbio_fm_filter_scan +
 * nvbio_fm_filter_locate_diagonals.  Capacities: seeds->n entries each.  counts_dev[0] = keys written, counts_dev[1] =
 * residual seeds (zeroed by the call).  The set of keys equals that of the plain operators over the same seeds.
 * seeds->n must be a whole number of strings (n = strings x seeds_per_string).
 * flags: NVBIO_FM_SCAN_FORWARD / NVBIO_FM_COMPLEMENT / NVBIO_FM_NO_KMER_TABLE as nvbio_fm_match; bits 16..31, if non-zero, cap
 * the launch at that many x 64 workgroups (a tuning / testing knob: results do not depend on it).
 * NVBIO_FM_COUNT_SECTORS: same results, and counts_dev (then 4 words, 8-byte aligned) also receives, as a uint64 in words
 * 2..3, the number of distinct 64-byte sectors the searches gathered from the index arrays (table entry, group, bwt_occ
 * records, SA word, text words): the unit in which the pass's memory traffic is accounted (a slower kernel instantiation,
 * for measurement harnesses).
 * temp_dev / temp_bytes: optional caller scratch (nvbio_fm_match_seed_diagonals_temp_bytes); if NULL the library allocates and
 * frees scratch itself (blocks kept per stream: see "Conventions"). */
nvbio_status nvbio_fm_match_seed_diagonals_temp_bytes(const nvbio_string_set* seeds, uint64_t* bytes);
nvbio_status nvbio_fm_match_seed_diagonals(nvbio_fm_index_t index, const nvbio_string_set* seeds, uint32_t flags, uint32_t read_len,
                                           uint32_t strand, uint64_t* keys_dev, nvbio_uint2* residual_ranges_dev, uint32_t* residual_ids_dev,
                                           uint32_t* counts_dev, void* temp_dev, uint64_t temp_bytes, void* stream);

/* Both strands of every seed in ONE pass (handles built with NVBIO_FM_TABLE_CANONICAL): the outputs of
 *   nvbio_fm_match_seed_diagonals( flags = 0, strand = 0 )  and
 *   nvbio_fm_match_seed_diagonals( flags = NVBIO_FM_SCAN_FORWARD | NVBIO_FM_COMPLEMENT, strand = 1 )
 * i.e. match() of every seed and of its reverse complement (nvBowtie maps both, mapping_inl.h:288-414) + locate() of the searches that end
 * on one row + hit_to_diagonal + the adjacent-duplicate removal, from one table gather per seed window: a k-mer and its reverse
 * complement share an entry that lists the occurrences of both orientations with the text on either side of each.
 *   keys_dev[0 .. counts_dev[0])        diagonal keys of both strands (read << 34 | strand << 33 | diagonal + 1024), grouped by tile of
 *                                       reads: a tile's forward keys in seed order, then its reverse-strand keys in seed order
 *   residual_*_dev[0 .. counts_dev[1])                              forward-strand searches that ended on several rows (range, seed id)
 *   residual_*_dev[residual_capacity .. + counts_dev[2])            the same for the reverse strand
 * keys_dev: nvbio_fm_match_seed_diagonals_both_keys_capacity() entries (256 per tile of 64 / seeds_per_string reads: with
 * NVBIO_FM_INLINE_HITS a seed can leave several keys, a tile at most 64 per strand -- slightly more than 2 * seeds->n when 64 is not a
 * multiple of seeds_per_string); residual arrays: 2 * residual_capacity entries, residual_capacity >= seeds->n.  counts_dev: 4 uint32
 * (6, 8-byte aligned, with NVBIO_FM_COUNT_SECTORS: the distinct 64-byte sectors gathered from the index as a uint64 at counts_dev + 4).
 * Seeds: packed 2 or 4 bits, fixed length in [kmer_len, kmer_len + 7], at most 64 per read.  flags: NVBIO_FM_COUNT_SECTORS, the grid
 * knob (bits 16..31) of nvbio_fm_match_seed_diagonals, and NVBIO_FM_INLINE_HITS(h), h in 2..4: a search that ends on up to h rows leaves
 * ALL their diagonal keys in keys_dev (behind its tile's one-row keys, no duplicate removal) instead of a residual entry -- what
 * FMIndexFilter's scan + locate would add for it, without the trip; only larger ranges reach the residual lists. */
#define NVBIO_FM_INLINE_HITS(h) (((uint32_t)(h) & 15u) << 8)
/* NVBIO_FM_DEFER_HEAVY: the searches the table cannot answer (a k-mer with more than 8 occurrences; more hits on a strand than
 * NVBIO_FM_INLINE_HITS) do not run inside the pass -- where every wave that holds one such window waits for its ten dependent gathers --
 * but are collected and run as a dense launch of their own behind it: same keys and residual entries (their keys follow the others in
 * keys_dev, without the adjacent-duplicate removal).  For repeat-rich references; on a unique-ish one it costs three short launches.
 * Ragged reads (seeds->seed_intervals_dev): read_len is ignored, every read's length comes from its offsets. */
#define NVBIO_FM_DEFER_HEAVY 64u
/* The locus path.  Where the handle keeps seed locus lines for seeds->fixed_len (nvbio_fm_index_seed_locus) and read_len <= 193 (ragged
 * reads: read by read), only a read's FIRST seed gathers its table entry at once; if it has exactly one hit over both strands, every
 * other seed of the read is compared with the text on that hit's diagonal in the read's one locus line, and is settled without a table
 * gather where the text equals it and u = 1 there -- which proves that the table would have answered with that one hit.  All other
 * seeds gather and resolve as ever: same keys, residual and deferred entries, in the same order.
 * NVBIO_FM_NO_SEED_LOCUS: the pass without that path (A/B measurements, tests).
 * NVBIO_FM_COUNT_LOCUS (with NVBIO_FM_COUNT_SECTORS only): counts_dev has 10 words; words 6..9 = reads whose first seed placed them |
 * seeds settled on the locus | seeds of such reads that gathered after all | seeds of the other reads (the last three over the seeds
 * behind a read's first; all zero where the path is off).  The sectors of NVBIO_FM_COUNT_SECTORS count a read's locus line once. */
#define NVBIO_FM_NO_SEED_LOCUS 128u
#define NVBIO_FM_COUNT_LOCUS 4096u
/* How a tile of reads is resolved.  A tile in which no seed has a k-mer with more than 8 occurrences and every seed ends on at most one
 * hit over both strands -- nearly every tile of a unique-ish genome -- is resolved by counting hits and emits the keys of both strands in
 * one pass; every other tile takes the general code (several hits on a strand, residual and deferred entries, in-line searches).  Same
 * keys, in the same order, either way.
 * The common way exists where it was measured to pay and costs no occupancy: 4-bit reads, 16-byte entries (NVBIO_FM_TABLE_CANONICAL_WIDE)
 * and NVBIO_FM_DEFER_HEAVY, with the locus path or without.  Every other launch -- 2-bit reads, 8-byte entries, no NVBIO_FM_DEFER_HEAVY (the
 * C++ host's) -- resolves every tile by the general code, as before.
 * NVBIO_FM_NO_FAST_RESOLVE: every tile takes the general code (A/B measurements, tests).  (Bits 8..11 belong to NVBIO_FM_INLINE_HITS.)
 * NVBIO_FM_COUNT_RESOLVE (with NVBIO_FM_COUNT_LOCUS only): counts_dev has 12 words; word 10 = tiles resolved on the common path, word
 * 11 = tiles resolved by the general code.  A flag of its own, so that a caller of NVBIO_FM_COUNT_LOCUS keeps its 10 words.  The accounting
 * launch reports what the launch of the same flags does: pass NVBIO_FM_DEFER_HEAVY with it to account for a launch with that flag (the
 * accounting launch itself defers nothing); without it word 10 is 0, as the launch it stands for has no common way. */
#define NVBIO_FM_NO_FAST_RESOLVE 8192u
#define NVBIO_FM_COUNT_RESOLVE 16384u
nvbio_status nvbio_fm_match_seed_diagonals_both_temp_bytes(const nvbio_string_set* seeds, uint64_t* bytes);
nvbio_status nvbio_fm_match_seed_diagonals_both_keys_capacity(const nvbio_string_set* seeds, uint64_t* n_keys);
nvbio_status nvbio_fm_match_seed_diagonals_both(nvbio_fm_index_t index, const nvbio_string_set* seeds, uint32_t flags, uint32_t read_len,
                                                uint64_t* keys_dev, nvbio_uint2* residual_ranges_dev, uint32_t* residual_ids_dev,
                                                uint32_t residual_capacity, uint32_t* counts_dev, void* temp_dev, uint64_t temp_bytes,
                                                void* stream);
/* The same pass with the tiles' spans kept: tile t (nvbio_fm_seed_tiles: reads_per_tile = 64 / seeds_per_string consecutive reads,
 * n_tiles = ceil( reads / reads_per_tile )) owns keys_dev[tile_offsets_dev[t] .. tile_offsets_dev[t + 1]): its forward-strand keys, then its
 * reverse-strand keys, every one of a read in [t * reads_per_tile, (t + 1) * reads_per_tile).  tile_offsets_dev: n_tiles + 1 uint32 (the
 * exclusive scan of the per-tile key counts the compaction runs anyway, NULL: not kept); counts_dev[3] = tile_offsets_dev[n_tiles], the
 * number of keys in tile order.  The keys NVBIO_FM_DEFER_HEAVY appends, [counts_dev[3], counts_dev[0]), belong to no tile's span: a
 * consumer that relies on the tile order (nvbio_finish_reads) needs counts_dev[3] == counts_dev[0]. */
nvbio_status nvbio_fm_seed_tiles(const nvbio_string_set* seeds, uint32_t* reads_per_tile, uint32_t* n_tiles);
nvbio_status nvbio_fm_match_seed_diagonals_both_tiled(nvbio_fm_index_t index, const nvbio_string_set* seeds, uint32_t flags, uint32_t read_len,
                                                      uint64_t* keys_dev, nvbio_uint2* residual_ranges_dev, uint32_t* residual_ids_dev,
                                                      uint32_t residual_capacity, uint32_t* counts_dev, uint32_t* tile_offsets_dev,
                                                      void* temp_dev, uint64_t temp_bytes, void* stream);
/* the k of the canonical two-strand table the handle holds (built with NVBIO_FM_TABLE_CANONICAL: it serves seeds of k .. k + 7 symbols),
 * 0 if it holds none */
int nvbio_fm_index_is_canonical(nvbio_fm_index_t index);

/* the two-phase form nvBowtie uses (locate_init / locate_lookup kernels, locate_inl.h:144-201):
 * jt_dev[i] = locate_ssa_iterator(rows[i]) = (sampled row, steps)  (fmindex_inl.h:404-437)
 * pos_dev[i] = lookup_ssa_iterator(jt[i]) = ssa[j/sa_int] + t      (fmindex_inl.h:445-460)
 * (the intermediate pair equals the reference's only for sa_int = 16; positions always do)      */
nvbio_status nvbio_fm_locate_init(nvbio_fm_index_t index, const uint32_t* rows_dev, uint32_t n,
                                  nvbio_uint2* jt_dev, void* stream);
nvbio_status nvbio_fm_locate_lookup(nvbio_fm_index_t index, const nvbio_uint2* jt_dev, uint32_t n,
                                    uint32_t* pos_dev, void* stream);

/* FMIndexFilter<device_tag>::rank (nvbio/fmindex/filter_inl.h:261-293): ranges + inclusive scan of
 * the range sizes (uint64).  *n_hits receives the total (host value; this call synchronizes). */
nvbio_status nvbio_fm_filter_rank(nvbio_fm_index_t index, const nvbio_string_set* queries, uint32_t flags,
                                  nvbio_uint2* ranges_dev, uint64_t* slots_dev, uint64_t* n_hits, void* stream);
/* the second half of FMIndexFilter::rank on its own (filter_inl.h:279-292): the inclusive scan of the sizes of
 * ranges that are already in HBM (e.g. from nvbio_fm_match) and the total; synchronizes like filter_rank. */
nvbio_status nvbio_fm_filter_scan(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, uint32_t n_queries,
                                  uint64_t* slots_dev, uint64_t* n_hits, void* stream);
/* FMIndexFilter<device_tag>::locate (filter_inl.h:299-393): hits_dev[h-begin] = (text_pos, query_id)
 * for the global hit indices h in [begin, end). */
nvbio_status nvbio_fm_filter_locate(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev,
                                    uint32_t n_queries, uint64_t begin, uint64_t end,
                                    nvbio_uint2* hits_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * SMEM seeding: MEMFilter<device_tag, fm_index> (nvbio/fmindex/mem.h, mem_inl.h:1303-1528) over a forward index and the
 * index of the reversed text (csrc/mem.hip).
 *
 * rank finds, for every read, its maximal exact matches in the reference's passes: right (forward extension with the reverse
 * index from x = 0, x = max(end, x + 1)), left (backward extension with the forward index), discard (per group, in entry order:
 * keep iff span begin < the left-most begin kept so far, span length >= min_span and occurrences <= max_intv; the device
 * filter's rule -- the marker moves only for kept MEMs), and, when split_len < 0xFFFFFFFF, split (a kept MEM with span >=
 * split_len and occurrences <= split_width is replaced by the forward extension from its midpoint with min_intv = occurrences
 * + 1, then left and discard again).  Reads are plain string sets (2-, 4- or 8-bit, symbols > 3 are N) of at most 65535 symbols.
 *
 * Departures from the reference (its defects):
 *   - ranges are exact SA intervals of their spans: the reference's extend_forward leaves out the suffix P$, which puts its
 *     forward ranges one row low;
 *   - span begins are not masked to 8 bits (the reference's MEMRange::span() is wrong from 256 symbols on);
 *   - inside a read the ranges are in ascending (span begin, span end) order (the reference leaves each read's last group
 *     unreversed);
 *   - nothing is dropped for capacity: a short buffer fails with NVBIO_ERR_INVALID and a message naming the size needed.
 * Working storage is the caller's temp only.
 * ------------------------------------------------------------------------------------------- */

/* MEMRange<uint32>: SA range [x, y], string id | 0x80000000 on the first kept MEM of a group, span begin | span end << 16 */
typedef struct { uint32_t x, y, string_id, span; } nvbio_mem_range;
/* MEMHit<uint32>: text position, string id, span [begin, end) */
typedef struct { uint32_t pos, string_id, span_begin, span_end; } nvbio_mem_hit;
/* the reference's defaults (mem.h:306-314): min_intv 1, max_intv 0xFFFFFFFF, min_span 1, split_len 0xFFFFFFFF (no split),
 * split_width 0xFFFFFFFF */
typedef struct { uint32_t min_intv, max_intv, min_span, split_len, split_width; } nvbio_mem_params;

/* the temp bytes nvbio_mem_filter_rank needs for these reads (a ragged set's offsets are read from the device: synchronizes) */
nvbio_status nvbio_mem_filter_temp_bytes(const nvbio_string_set* reads, const nvbio_mem_params* params, uint64_t* bytes, void* stream);
/* MEMFilter::rank.  ranges_dev / slots_dev: max_ranges entries; first_range_dev: reads->n + 1 entries, first_range[i] = index of
 * string i's first range (first_hit(i) = slots[first_range[i] - 1], 0 for the first).  slots = inclusive scan (uint64) of the range
 * sizes.  *n_ranges, *n_mems (host) = ranges and MEM occurrences; *records (optional, host) = the 32-byte bwt_occ records the
 * passes gathered.  f_index and r_index must have the same length and L2 (NVBIO_ERR_INVALID otherwise); seed-enumerated sets are
 * rejected.  max_ranges too small: NVBIO_ERR_INVALID, *n_ranges = the number needed.  temp too small (the split pass may need more
 * than nvbio_mem_filter_temp_bytes): NVBIO_ERR_INVALID, the message names the bytes needed.  Either failure is found only after
 * the passes before it have run, and a rerun repeats every pass: without split, max_ranges = the reads' symbol total (a read has at
 * most one range per symbol) and the temp of nvbio_mem_filter_temp_bytes always suffice; with split, keep the sizes a call needed
 * for the next batch (the mirrors do).  Synchronizes. */
nvbio_status nvbio_mem_filter_rank(nvbio_fm_index_t f_index, nvbio_fm_index_t r_index, const nvbio_string_set* reads,
                                   const nvbio_mem_params* params, nvbio_mem_range* ranges_dev, uint32_t max_ranges,
                                   uint32_t* first_range_dev, uint64_t* slots_dev, void* temp_dev, uint64_t temp_bytes,
                                   uint32_t* n_ranges, uint64_t* n_mems, uint64_t* records, void* stream);
/* MEMFilter::locate: hits_dev[h - begin] for the MEM occurrences h in [begin, end), end <= *n_mems (checked: reads slots, synchronizes) */
nvbio_status nvbio_mem_filter_locate(nvbio_fm_index_t f_index, const nvbio_mem_range* ranges_dev, const uint64_t* slots_dev,
                                     uint32_t n_ranges, uint64_t begin, uint64_t end, nvbio_mem_hit* hits_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * q-gram seeding: QGramIndexDevice, QGramSetIndexDevice and QGramFilter<device_tag> (nvbio/qgram/qgram.h, qgram_inl.h,
 * filter.h, filter_inl.h; csrc/qgram.hip), the pieces of examples/qmap/qmap.cu.  No BWT and no suffix array: a q-gram index is
 * the sorted unique q-grams of a text (or of the seeds of a string set), their slots and their occurrences.
 *
 *   packing  g = sum_j (s[i+j] & mask) << (j * symbol_size), mask = (1 << symbol_size) - 1: the FIRST symbol in the LEAST
 *            significant bits (numeric order is not lexicographic order), positions past the end of the string give 0 symbols, and
 *            a 4-bit N (4) read with symbol_size 2 becomes A (qmap relies on it).
 *   string   all `length` positions are indexed, the last q - 1 padded with 0 symbols (n_qgrams = length); the occurrences of a
 *            q-gram are uint32 text positions in ascending order (a stable radix sort over bits [0, q * symbol_size)).
 *   set      seeds at pos = k * seed_interval for every k with pos + q <= the string's length (no padding), string-major then by
 *            position; coordinates (string_id, string_pos), uint32 each, in that order inside a q-gram.
 *   view     qgrams[n_unique] sorted unique q-grams; slots[n_unique + 1] exclusive scan of their counts; index[n_qgrams] the
 *            occurrences; lut[A^qlut + 1] (qlut > 0, A = 1 << symbol_size): lut[k] = lower_bound( qgrams, k << (q - qlut) *
 *            symbol_size ), lut[A^qlut] = n_unique -- it keys on a q-gram's top bits, its LAST qlut symbols.
 *   range    the HALF-OPEN occurrence range [slots[i], slots[i+1]) of g, (0, 0) on a miss (the FM ranges above are inclusive).
 *   rank     ranges[i] = range( qgrams[i] ); slots = INCLUSIVE uint64 scan of the range sizes; *n_hits = slots[n - 1].
 *   locate   output o belongs to query i = upper_bound( o, slots ).  String index: hits are uint2 (index[ranges[i].x + o -
 *            slots[i-1]], indices[i]) = (text position of the occurrence, the caller's coordinate of query i); set index: uint4
 *            (string_id, string_pos, indices[i], 0).
 *   merge    diagonal = text_pos - index_pos (string hits: hit.y - hit.x) or text_pos - string_pos (set hits: hit.z - hit.y), uint32
 *            (it wraps), snapped to the closest multiple of interval (ties down, mod 2^32), sorted and run-length encoded: string
 *            hits give uint32 diagonals, set hits uint2 (diagonal, string_id) ordered by string id, then diagonal; counts uint32.
 *
 * Departures from the reference (its defects): util::round returns r + 1 instead of the closest multiple r + interval; rank over
 * no queries returns 0 hits (the reference reads slots[-1]); the set-index locate keeps the hit index 64-bit (the reference
 * truncates it to 32 bits); merged counts are uint32 (qmap's uint16 can overflow on a repeat).
 * Limits (NVBIO_ERR_INVALID otherwise): 1 <= symbol_size <= 8, q >= 1, q * symbol_size <= 64, qlut <= q, qlut * symbol_size <=
 * 28; text lengths and n_qgrams below 2^32 - 1; text / symbol bits 2, 4 or 8 (the nvbio_string_set packing).
 * Working storage: the builds allocate their own (the arrays stay with the handle); generate (sorted), rank and merge use the
 * caller's temp only.
 * ------------------------------------------------------------------------------------------- */
typedef struct nvbio_qgram_index_s* nvbio_qgram_index_t;     /* opaque handle */

typedef struct
{
    uint32_t        q, symbol_size, qlut;
    uint32_t        is_set;            /* 0: string index (index = uint32 positions); 1: set index (index = uint2 coordinates) */
    uint32_t        n_qgrams, n_unique;
    uint64_t        lut_size;          /* A^qlut (lut_dev holds lut_size + 1 entries), 0 without a LUT */
    int             device;
    const uint64_t* qgrams_dev;
    const uint32_t* slots_dev;
    const void*     index_dev;
    const uint32_t* lut_dev;           /* NULL without a LUT */
} nvbio_qgram_index_view;

/* QGramIndexDevice::build( q, symbol_size, length, text, qlut ): text_dev packed as nvbio_string_set symbols (big-endian words of
 * 2 or 4 bits, or bytes).  Synchronizes. */
nvbio_status nvbio_qgram_index_build(int device, const void* text_dev, uint32_t text_bits, uint32_t length, uint32_t q, uint32_t symbol_size,
                                     uint32_t qlut, nvbio_qgram_index_t* out, void* stream);
/* QGramSetIndexDevice::build( q, symbol_size, set, uniform_seeds_functor( q, seed_interval ), qlut ) over a plain string set (fixed,
 * ragged, or offsets not starting at 0); seed-enumerated sets are rejected.  Synchronizes. */
nvbio_status nvbio_qgram_set_index_build(int device, const nvbio_string_set* set, uint32_t q, uint32_t symbol_size, uint32_t seed_interval,
                                         uint32_t qlut, nvbio_qgram_index_t* out, void* stream);
nvbio_status nvbio_qgram_index_destroy(nvbio_qgram_index_t index);
nvbio_status nvbio_qgram_index_get_view(nvbio_qgram_index_t index, nvbio_qgram_index_view* view);
nvbio_status nvbio_qgram_index_device_bytes(nvbio_qgram_index_t index, uint64_t* bytes);
/* copy the index arrays into caller buffers in HBM (any may be NULL; sizes from get_view: n_unique, n_unique + 1, n_qgrams entries of
 * uint32 or uint2, lut_size + 1) */
nvbio_status nvbio_qgram_index_export(nvbio_qgram_index_t index, uint64_t* qgrams_out_dev, uint32_t* slots_out_dev, void* index_out_dev,
                                      uint32_t* lut_out_dev, void* stream);

/* qmap's build_qgrams (examples/qmap/qmap.cu:75-99): qgrams_dev[i] = the q-gram at text position first_pos + i for i < n (padded
 * past text_len), indices_dev[i] = first_pos + i (indices_dev may be NULL when !sort).  sort != 0: the (q-gram, position) pairs
 * stably sorted by q-gram, in the caller's temp (nvbio_generate_qgrams_temp_bytes; none without sort). */
nvbio_status nvbio_generate_qgrams_temp_bytes(uint32_t n, int sort, uint64_t* bytes);
nvbio_status nvbio_generate_qgrams(int device, uint32_t q, uint32_t symbol_size, const void* text_dev, uint32_t text_bits, uint32_t text_len,
                                   uint32_t first_pos, uint32_t n, uint64_t* qgrams_dev, uint32_t* indices_dev, int sort,
                                   void* temp_dev, uint64_t temp_bytes, void* stream);
/* the index as a search functor: ranges_dev[i] = range( qgrams_dev[i] ) */
nvbio_status nvbio_qgram_ranges(nvbio_qgram_index_t index, const uint64_t* qgrams_dev, uint32_t n, nvbio_uint2* ranges_dev, void* stream);

/* QGramFilter::rank: ranges_dev / slots_dev hold n entries; temp: nvbio_qgram_filter_temp_bytes( n ).  Synchronizes. */
nvbio_status nvbio_qgram_filter_temp_bytes(uint32_t n_queries, uint64_t* bytes);
nvbio_status nvbio_qgram_filter_rank(nvbio_qgram_index_t index, const uint64_t* qgrams_dev, uint32_t n, nvbio_uint2* ranges_dev, uint64_t* slots_dev,
                                     void* temp_dev, uint64_t temp_bytes, uint64_t* n_hits, void* stream);
/* QGramFilter::locate: hits_dev[o - begin] for the outputs o in [begin, end), end <= slots[n - 1] (checked: reads it, synchronizes);
 * uint2 hits for a string index, uint4 for a set index.  indices_dev: the query coordinates rank's queries came with (n entries). */
nvbio_status nvbio_qgram_filter_locate(nvbio_qgram_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev, const uint32_t* indices_dev,
                                       uint32_t n, uint64_t begin, uint64_t end, void* hits_dev, void* stream);
/* QGramFilter::merge: merged_dev (n_hits uint32, or uint2 when is_set) and counts_dev (n_hits uint32) receive *n_merged entries;
 * temp: nvbio_qgram_filter_merge_temp_bytes( is_set, n_hits ).  interval >= 1.  Synchronizes. */
nvbio_status nvbio_qgram_filter_merge_temp_bytes(int is_set, uint32_t n_hits, uint64_t* bytes);
nvbio_status nvbio_qgram_filter_merge(int device, int is_set, uint32_t interval, const void* hits_dev, uint32_t n_hits, void* merged_dev,
                                      uint32_t* counts_dev, uint32_t* n_merged, void* temp_dev, uint64_t temp_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * the q-group index: QGroupIndexDevice (the PEANUT structure; nvbio/qgram/qgroup.h:60-290, qgroup_inl.h:28-277;
 * csrc/qgroup_inl.h), the O(1)-lookup alternative to the sorted q-gram index above (nvbio/qgram/qgram.h:76-88), in a string and
 * a set form.  A bit table addressed by the q-gram itself replaces the search, so a range lookup is two dependent loads whatever
 * the text size.  The handle is an nvbio_qgram_index_t: nvbio_qgram_index_destroy, nvbio_qgram_index_device_bytes,
 * nvbio_qgram_ranges, nvbio_qgram_filter_rank and nvbio_qgram_filter_locate take it unchanged in signature and meaning.
 *
 * With A = 1 << symbol_size and W = A^q / 32 (integer division):
 *   I        W + 1 words; bit (g & 31) of word g / 32 is set iff q-gram g occurs.
 *   S        W + 1 words; the exclusive scan of popc( I[i] ).
 *   SS       n_unique + 1 words; the exclusive scan of the occurrence counts of the unique q-grams in ascending numeric order;
 *            SS[n_unique] = n_qgrams.
 *   P        n_qgrams coordinates: uint32 positions (string index), uint2 (string_id, string_pos) (set index).
 *   range    (0, 0) if the bit of g is clear; else the HALF-OPEN (SS[S[i] + j'], SS[S[i] + j' + 1]) with i = g / 32, j = g & 31,
 *            j' = popc( I[i] & ((1 << j) - 1) ) (qgroup.h:112-130).
 *   table    I[i] and S[i] are kept interleaved as uint2 (I[i], S[i]), so the first step of a lookup is one 8-byte load; export
 *            hands them out as the reference's two arrays.
 * Packing, padding (string: every position, the tail padded; set: uniform_seeds_functor( q, seed_interval ), no padding) and
 * N -> A are exactly those of the q-gram index.
 *
 * Departures from the reference:
 *   order    the reference's fill takes slots with a returning atomic, so the order of a q-gram's occurrences in P is whatever the
 *            scheduler made it.  Here it is defined: ascending position (string index); string-major, then position (set index).
 *            For the same input SS equals the q-gram index's slots, P its index, the set bits of I its qgrams, and two builds
 *            give identical bytes.
 *   range    range( g ) for g >= A^q is a miss (the reference reads I out of bounds).
 *   n_unique S[W] + popc( I[W] ); the reference takes S[W], which is 0 when q * symbol_size < 5 (W = 0: the one word holds every
 *            bit).  For q * symbol_size >= 5 word W holds no bit and S[W] = n_unique.
 *   empty    an empty text or set builds (n_unique = 0, SS = {0}); the reference has no set form.
 * Limits (NVBIO_ERR_INVALID otherwise): 1 <= symbol_size <= 8, q >= 1, q * symbol_size <= 36 (the word index still fits uint32; the
 * table is then 16 GiB -- qmap's Q = 20 at two bits would need 2^40 bits and is outside); n_qgrams below 2^32 - 1; text / symbol
 * bits 2, 4 or 8.  A table that does not fit in HBM gives NVBIO_ERR_NOMEM.
 * Working storage: the builds allocate their own (the table, SS and P stay with the handle).
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t           q, symbol_size;
    uint32_t           is_set;         /* 0: string index (P = uint32 positions); 1: set index (P = uint2 coordinates) */
    uint32_t           n_qgrams, n_unique;
    uint64_t           n_words;        /* W + 1: the entries of table_dev */
    int                device;
    const nvbio_uint2* table_dev;      /* (I[i], S[i]) */
    const uint32_t*    ss_dev;         /* n_unique + 1 */
    const void*        p_dev;          /* n_qgrams */
} nvbio_qgroup_index_view;

/* QGroupIndexDevice::build( q, symbol_size, length, text ) (qgroup_inl.h:162-277): text_dev packed as nvbio_string_set symbols.
 * Synchronizes. */
nvbio_status nvbio_qgroup_index_build(int device, const void* text_dev, uint32_t text_bits, uint32_t length, uint32_t q, uint32_t symbol_size,
                                      nvbio_qgram_index_t* out, void* stream);
/* the set form over a plain string set, seeded as nvbio_qgram_set_index_build.  Synchronizes. */
nvbio_status nvbio_qgroup_set_index_build(int device, const nvbio_string_set* set, uint32_t q, uint32_t symbol_size, uint32_t seed_interval,
                                          nvbio_qgram_index_t* out, void* stream);
/* NVBIO_ERR_INVALID on a sorted q-gram index.  (nvbio_qgram_index_get_view on a q-group handle fills the common fields with
 * slots_dev = SS, index_dev = P, qgrams_dev = lut_dev = NULL and qlut = 0; nvbio_qgram_index_export on one is NVBIO_ERR_INVALID.) */
nvbio_status nvbio_qgroup_index_get_view(nvbio_qgram_index_t index, nvbio_qgroup_index_view* view);
/* copy I and S (n_words uint32 each, the reference's layout), SS (n_unique + 1) and P (n_qgrams uint32 or uint2) into caller buffers
 * in HBM; any may be NULL */
nvbio_status nvbio_qgroup_index_export(nvbio_qgram_index_t index, uint32_t* I_out_dev, uint32_t* S_out_dev, uint32_t* SS_out_dev, void* P_out_dev,
                                       void* stream);

/* -------------------------------------------------------------------------------------------
 * sufsort: the suffix sort and the BWT of a string set and of a string (nvbio/sufsort/sufsort.h: cuda::suffix_sort( string_set ),
 * cuda::bwt( string_set ), the engine of nvSetBWT; cuda::suffix_sort( string ), cuda::bwt( string ), find_primary).
 * csrc/sufsort.hip (sets), csrc/fm_build.hip (strings).
 *
 * String sets (plain sets of N strings of lengths len_i, in any form of nvbio_string_set; seed enumerations are rejected):
 *   suffix   (pos, string_id) with 0 <= pos <= len_i; pos == len_i is the empty suffix.
 *   order    by raw symbol value (the whole symbol_bits-wide symbol); a suffix that is a proper prefix of another sorts first (the
 *            implicit '$', below every symbol); suffixes equal up to and including their ends sort by ascending string_id.  Hence
 *            the N empty suffixes come first, in string order (sufsort_inl.h:70-135: a stable LSD sort from string-major order with
 *            SetSuffixFlattener's empty suffixes; sufsort_inl.h:535-560: the "dollar" block first).
 *   bwt      bwt[r] = the symbol in front of the r-th sorted suffix, 255 when pos == 0 (string_set_bwt_functor,
 *            sufsort_priv.h:881-904); one byte per suffix, sum( len_i + 1 ) of them.
 *   flag     NVBIO_SUFSORT_NO_EMPTY_SUFFIXES drops the N empty suffixes from every output: sum( len_i ) entries.
 *   global   the reference's global suffix index (what its SuffixHandler consumes): pos + the exclusive sum of (len_j + 1), or of
 *            len_j under the flag, over the strings j before string_id.
 * Departures from the reference: the method.  The reference sorts all suffixes once per 14-symbol word, least significant word
 * first; this library sorts the first word once and refines only the suffixes that still tie (csrc/sufsort.hip).  The order is the
 * one stated above in every case, and two calls give equal bytes.
 * Limits (NVBIO_ERR_INVALID otherwise): symbol_bits 2, 4 or 8; sum( len_i + 1 ) < 2^32 - 1, with or without the flag; N = 0 and
 * strings of length 0 are valid.  Out of scope: the reference's host-memory-bounded large_bwt, its BWT file writers, and an
 * FM-index over a read set.
 * Working storage: each call allocates its own and frees it before it returns; each call synchronizes.  An output capacity (in
 * suffixes) below the count fails with the needed size in nvbio_amd_last_error, before any sort work.
 *
 * Strings (2-bit big-endian packed texts, as nvbio_fm_index_build takes them): the sorter of the index build, with repeats of up to
 * 2^20 symbols.
 * ------------------------------------------------------------------------------------------- */
enum { NVBIO_SUFSORT_NO_EMPTY_SUFFIXES = 1 };

/* the work a set sort did, so that tests and benchmarks can see it without timing it */
typedef struct
{
    uint32_t n_suffixes;
    uint32_t rounds;                /* sorts run: round 0 over every suffix, round k > 0 over the suffixes still tied after k words */
    uint32_t sorted_per_round[16];  /* the suffixes that entered round k's sort (the first 16 rounds) */
    uint32_t symbols_per_word;      /* 29 (2-bit), 15 (4-bit) or 7 (8-bit) symbols per 64-bit key word */
    uint64_t peak_bytes;            /* the most device memory the call held at once, outputs excluded */
} nvbio_sufsort_stats;

/* the number of suffixes the two calls below write */
nvbio_status nvbio_set_suffix_count(int device, const nvbio_string_set* set, uint32_t flags, uint32_t* n_suffixes, void* stream);
/* suffixes_dev[r] = (pos, string_id) of the r-th suffix, global_dev[r] (may be NULL) its global index; both hold `capacity` entries.
 * stats may be NULL. */
nvbio_status nvbio_set_suffix_sort(int device, const nvbio_string_set* set, uint32_t flags, nvbio_uint2* suffixes_dev, uint32_t* global_dev,
                                   uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream);
/* the same sort in the form the reference's suffix handler takes (process( n_suffixes, suffix_array, string_ids, cum_lengths )), all in
 * device memory: suffix_array_dev[r] = the global index of the r-th suffix, string_ids_dev[r] (may be NULL) its string, both of `capacity`
 * entries; cum_lengths_dev[i] (may be NULL, set->n entries) = the suffixes of the strings up to and including i. */
nvbio_status nvbio_set_suffix_sort_flat(int device, const nvbio_string_set* set, uint32_t flags, uint32_t* suffix_array_dev, uint32_t* string_ids_dev,
                                        uint32_t* cum_lengths_dev, uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream);
/* bwt_dev[r] = the symbol in front of the r-th suffix (255 in front of a string), suffixes_dev (may be NULL) as above */
nvbio_status nvbio_set_bwt(int device, const nvbio_string_set* set, uint32_t flags, uint8_t* bwt_dev, nvbio_uint2* suffixes_dev,
                           uint64_t capacity, uint32_t* n_suffixes, nvbio_sufsort_stats* stats, void* stream);

/* cuda::suffix_sort( string ): sa_dev[length + 1], the suffix array in the convention of nvbio/fmindex/bwt.h:28-37 (row 0 = the empty
 * suffix, sa_dev[0] = length).  length > 0.  Repeats of up to 2^20 symbols are sorted (the most the sorter's doubling rounds take; the
 * index build's default of 4096 does not apply here); a text with a longer one is NVBIO_ERR_UNSUPPORTED.  Synchronizes. */
nvbio_status nvbio_suffix_sort(const uint32_t* text2_dev, uint32_t length, int device, uint32_t* sa_dev, void* stream);
/* cuda::bwt( string ) and find_primary: bwt_words_dev[ceil( length / 16 )], the BWT 2-bit big-endian packed with the primary row
 * squeezed out (bwt.h:41-53) -- exactly the words nvbio_fm_index_build interleaves with its occurrence counts -- and *primary, the
 * row of '$'.  Synchronizes. */
nvbio_status nvbio_bwt(const uint32_t* text2_dev, uint32_t length, int device, uint32_t* bwt_words_dev, uint32_t* primary, void* stream);

/* -------------------------------------------------------------------------------------------
 * seed hits -> candidate windows: the two index-arithmetic functors between FMIndexFilter::locate
 * and the banded aligner in the reference's smallest seed-and-extend caller (examples/fmmap/fmmap.cu)
 * ------------------------------------------------------------------------------------------- */

/* hit_to_diagonal (examples/fmmap/fmmap.cu:92-117) for uniformly enumerated seeds: for hit
 * (text_pos, seed_id), read = seed_id / seeds_per_read, seed offset p = (seed_id % seeds_per_read) *
 * seed_interval (on the reverse-complement strand p -> read_len - p - seed_len), diagonal = text_pos - p.
 * keys_dev[h] = read << 34 | strand << 33 | (diagonal + 1024): sortable, one per hit.
 * The field of the diagonal holds 33 bits and a bias of 1024, so a seed may lie at most NVBIO_MAX_SEED_OFFSET = 1024 symbols into its read:
 * a hit of a later seed within (offset - 1024) symbols of the genome start would leave the field below zero and spill over the strand
 * bit and the read id.  Every call that forms diagonal keys -- this one, nvbio_fm_filter_locate_diagonals, nvbio_fm_residual_diagonals,
 * nvbio_fm_match_seed_diagonals[_both[_tiled]] -- therefore refuses read_len - seed_len > NVBIO_MAX_SEED_OFFSET with NVBIO_ERR_INVALID.
 * Their ragged forms (read_offsets_dev on the device) cannot look at the lengths: there the limit is the CALLER's to keep, for the longest
 * read of the batch (pipeline.seed_and_extend checks it on the host).                                                              */
#define NVBIO_MAX_SEED_OFFSET 1024u
nvbio_status nvbio_hits_to_diagonals(int device, const nvbio_uint2* hits_dev, uint64_t n_hits, uint32_t seeds_per_read,
                                     uint32_t seed_interval, uint32_t seed_len, uint32_t read_len, uint32_t strand,
                                     uint64_t* keys_dev, void* stream);

/* Sort candidate keys and drop duplicates, in place: what fmmap does with its diagonals before extending them
 * (examples/fmmap/fmmap.cu:320-344: sort_by_key + unique), for host compositions that have no device sort of their own.
 * *n_out_dev (device) = number of distinct keys, left at the front of keys_dev in ascending order.
 * temp_dev / temp_bytes: optional caller scratch (nvbio_sort_unique_keys_temp_bytes). */
nvbio_status nvbio_sort_unique_keys_temp_bytes(uint64_t n, uint64_t* bytes);
nvbio_status nvbio_sort_unique_keys(int device, uint64_t* keys_dev, uint64_t n, uint32_t* n_out_dev, void* temp_dev, uint64_t temp_bytes, void* stream);

/* genome_infixes (examples/fmmap/fmmap.cu:169-196) with nvBowtie's window rule (BestScoreStream::init_context,
 * nvBowtie/bowtie2/cuda/score_inl.h:100-106): g_pos = max(diagonal,0); begin = g_pos > band/2 ? g_pos - band/2 : 0;
 * end = min(begin + band + read_len, genome_len); flags = strand ? REVERSE|COMPLEMENT : 0.                */
nvbio_status nvbio_diagonals_to_windows(int device, const uint64_t* keys_dev, uint64_t n, uint32_t band, uint32_t read_len,
                                        uint32_t genome_len, uint32_t* read_id_dev, uint8_t* flags_dev,
                                        uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream);

/* Ragged read batches (reads of different lengths: io::SequenceData's sequence_index; nvBowtie takes every read's length from its
 * range, mapping_inl.h:507-529, score_inl.h:100-106): the same operators with read_offsets_dev (n_reads + 1 symbol offsets) in place
 * of one read_len -- and, where a threshold depends on the read's length (MinScoreFunc, scoring.h:117-129), min_scores_dev[r] =
 * scheme.min_score( length of read r ) computed by the caller. */
nvbio_status nvbio_diagonals_to_windows_ragged(int device, const uint64_t* keys_dev, uint64_t n, uint32_t band, const uint32_t* read_offsets_dev,
                                               uint32_t genome_len, uint32_t* read_id_dev, uint8_t* flags_dev,
                                               uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream);
nvbio_status nvbio_fm_filter_locate_diagonals_ragged(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, const uint64_t* slots_dev,
                                                     const uint8_t* direct_dev, uint32_t n_queries, uint64_t begin, uint64_t end,
                                                     uint32_t seeds_per_read, uint32_t seed_len, const uint32_t* read_offsets_dev,
                                                     const uint32_t* seed_intervals_dev, uint32_t strand, const uint32_t* query_ids_dev,
                                                     uint64_t* keys_dev, void* stream);
nvbio_status nvbio_traceback_best_batch_ragged(int device, const uint64_t* best_dev, const int64_t* best_wb_dev, uint32_t n_reads,
                                               const uint32_t* read_offsets_dev, uint32_t band, uint32_t genome_len, const int32_t* min_scores_dev,
                                               uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* scores_dev,
                                               nvbio_uint2* sinks_dev, void* stream);
/* distinct_dist = (length of the candidate's read) / 2, worst_score = min_scores_dev[read] - 1 */
nvbio_status nvbio_second_candidate_reduce_ragged(int device, const uint64_t* keys_dev, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                                  const uint32_t* win_begin_dev, uint64_t n, const uint64_t* best_dev,
                                                  const uint32_t* read_offsets_dev, const int32_t* min_scores_dev, uint64_t* second_dev, void* stream);
/* perfect_score = match x (length of the read), min_score = min_scores_dev[read], monotone = (match == 0) */
nvbio_status nvbio_mapq_ragged(int device, const uint64_t* best_dev, const uint64_t* second_dev, uint32_t n_reads, int32_t version, int32_t match,
                               const uint32_t* read_offsets_dev, const int32_t* min_scores_dev, int32_t* second_scores_dev, uint8_t* mapq_dev,
                               void* stream);

/* The residual seeds of a seed pass (nvbio_fm_match_seed_diagonals[_both]: searches that ended on several SA rows) under a seed-hit cap, in
 * ONE call: the first `cap` rows of every range (nvBowtie bounds repeats with its max_hits deque, mapping_inl.h:242-244; this is the order-free
 * stand-in the default pipeline uses) are located and turned into diagonal keys, as nvbio_fm_filter_scan + nvbio_fm_filter_locate_diagonals
 * over the capped ranges would -- without the scan, its host synchronisation and the global sort a duplicate removal would take: the
 * entries are sorted by seed id, so that consecutive seeds of a read are neighbours, and a key equal to the one the previous entry leaves
 * at the same row is dropped (the seeds of a read inside a repeat list the same loci row for row).  The SET of keys equals that of the
 * two-call form; a duplicate that survives costs a repeated extension, nothing else.
 *   ids_dev[e]        seed id of entry e, bit 31 = reverse strand (the convention of nvbio_fm_filter_locate_diagonals' query_ids_dev)
 *   keys_dev          room for n * cap keys; *n_keys_dev (device) = keys written
 *   read_offsets_dev / seed_intervals_dev   ragged reads (both or neither; then seed_interval and read_len are ignored)
 * Needs the full suffix array (sa_int = 1).  1 <= cap <= 64, n * cap < 2^31.  A call refused for its arguments writes nothing, *n_keys_dev included.
 * The ranges of real searches hold rows >= 1; row 0 (the empty suffix) is outside the contract: for it this call reports the position `length`,
 * the two-call form ssa[0] + t. */
nvbio_status nvbio_fm_residual_diagonals(nvbio_fm_index_t index, const nvbio_uint2* ranges_dev, const uint32_t* ids_dev, uint32_t n, uint32_t cap,
                                         uint32_t seeds_per_read, uint32_t seed_interval, uint32_t seed_len, uint32_t read_len,
                                         const uint32_t* read_offsets_dev, const uint32_t* seed_intervals_dev,
                                         uint64_t* keys_dev, uint32_t* n_keys_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * nvBowtie's scoring stream, as data: what a specialisation of aln::BatchedBandedAlignmentScore for
 * bowtie2::cuda::BestScoreStream (nvBowtie/bowtie2/cuda/score_inl.h:44-136) hands over instead of per-item callbacks.
 * The arrays are the members of the stream's pipeline object (pipeline_states.h:49-115, scoring_queues.h:211-289), all in HBM:
 *   idx_queue_dev    pipeline.idx_queue: work item i scores hit idx_queue[i] (NULL: hit i)            (score_inl.h:89)
 *   hit_read_id_dev  pipeline.scoring_queues.hits.read_id
 *   hit_seed_dev     pipeline.scoring_queues.hits.seed, one packed_seed word per hit (defs.h:162-172: pos_in_read:12,
 *                    index_dir:1, rc:1, top_flag:1 from bit 0; only rc is read)
 *   hit_loc_dev      pipeline.scoring_queues.hits.loc                                                  (score_inl.h:100)
 *   hit_score_dev / hit_sink_dev   pipeline.scoring_queues.hits.score / .sink: the stream's output   (score_inl.h:127-129)
 *   n                pipeline.hits_queue_size = stream.size()
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    const uint32_t* idx_queue_dev;
    uint32_t*       hit_read_id_dev;   /* written by nvbio_seed_hits_select, read by the scoring stream calls */
    uint32_t*       hit_seed_dev;
    uint32_t*       hit_loc_dev;
    int32_t*        hit_score_dev;
    uint32_t*       hit_sink_dev;
    uint32_t        n;
} nvbio_hit_queues;

/* BestScoreStream::init_context + the orientation of load_strings for every work item (score_inl.h:85-115, alignment_utils.h:277-302):
 * the four per-job arrays of an nvbio_alignment_batch.  read_index_dev = the read batch's sequence_index (n_reads + 1 symbol
 * offsets, io::SequenceData); band_len = the stream's m_band_len; genome_len = pipeline.genome_length; reads_reversed = 1 when
 * the read batch was loaded with io::REVERSE, as nvBowtie does (nvBowtie.cpp:322,337,356): a forward hit then reads the stored
 * stream backwards (NVBIO_READ_REVERSE) and a reverse-complemented one forwards, complemented (NVBIO_READ_COMPLEMENT).
 * (context->min_score = max(second best, score_limit) is not needed: whole-pattern banded scoring never reads it,
 * gotoh_banded_inl.h:610-622 is the windowed form only.) */
nvbio_status nvbio_score_stream_flatten(int device, const nvbio_hit_queues* hits, const uint32_t* read_index_dev, uint32_t band_len,
                                        uint32_t genome_len, uint32_t reads_reversed, uint32_t* read_id_dev, uint8_t* flags_dev,
                                        uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream);
/* BestScoreStream::output for every work item (score_inl.h:119-133): hit.score = max( score, worst_score ) (scheme_type::worst_score
 * = -65536, scoring.h:223-224), hit.sink = window begin + sink.x, scattered through idx_queue. */
nvbio_status nvbio_score_stream_output(int device, const nvbio_hit_queues* hits, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                       const uint32_t* win_begin_dev, int32_t worst_score, void* stream);

/* -------------------------------------------------------------------------------------------
 * nvBowtie's seed-hit bookkeeping (the data-parallel kernels of its best-approx extension loop, aligner_best_approx.h:453-666):
 * per-read deques of seed hits, the selection of the next SA row, the effort-limited best / second-best reduction.
 * One SeedHit = 8 bytes: x = range_begin, y = range_delta:20 | pos_in_read:10 | rc:1 | indexdir:1 (seed_hit.h:45-218; the SA range is
 * exclusive at its end).  A read's deque is the reference's priority_deque over an interval heap (nvbio/basic/priority_deque.h):
 * element 0 the largest range, element 1 the smallest; `capacity` entries per read, deque r at deques_dev + r * capacity.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t seeds_per_read;   /* seeds mapped per read and strand                                                               */
    uint32_t first_offset;     /* stored offset of seed 0: retry * (seed_freq / (max_reseed + 1))         (mapping_inl.h:520,528) */
    uint32_t seed_interval;    /* seed_freq( read_len )                                                                          */
    uint32_t seed_len;
    uint32_t read_len;         /* reads of one length (< 1024: SeedHit keeps positions in 10 bits)                               */
    uint32_t max_hits;         /* cap of the deque: a full deque drops its largest range before every push  (:242-244; default 100) */
    uint32_t rep_seeds;        /* reseed when the mean range size reaches this                              (:549; default 1000)    */
    uint32_t max_effort;       /* failed extensions in a row that end a read's search                       (reduce.h:72-97; 15)   */
    uint32_t min_ext;          /* ... counted only from this many extensions on                             (default 30)           */
    uint32_t max_ext;          /* hard limit of extensions per read                                         (default 400)          */
} nvbio_seed_hits_params;

/* entries per read a deque array needs for these parameters: min( 2 x seeds_per_read, max_hits ) + 1 */
nvbio_status nvbio_seed_hits_capacity(uint32_t seeds_per_read, uint32_t max_hits, uint32_t* capacity);

/* seed_mapper<EXACT_MAPPING>::enact + the bookkeeping of map_kernel (nvBowtie/bowtie2/cuda/mapping_inl.h:193-282,485-556) for reads whose
 * seeds have been matched: fw_ranges_dev / rc_ranges_dev [n_reads x seeds_per_read] = nvbio_fm_match over the seeds of the STORED
 * (reversed) reads with NVBIO_FM_SCAN_FORWARD, and with NVBIO_FM_COMPLEMENT (reverse scan) -- the two match_range calls of the
 * mapper (USE_REVERSE_INDEX 0).  Work item t is read read_queue_dev[t] (NULL: read t).  For every seed, forward hit then
 * reverse-complemented hit are pushed in the reference's order under its max_hits rule; sizes_dev[r] = hits kept;
 * reseed_dev[r] (optional) = the reseeding decision `range_count == 0 || range_sum >= rep_seeds * range_count`. */
nvbio_status nvbio_seed_hits_map(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, const uint32_t* read_queue_dev,
                                 uint32_t n_reads, const nvbio_seed_hits_params* params, nvbio_uint2* deques_dev, uint32_t* sizes_dev,
                                 uint8_t* reseed_dev, void* stream);

/* nvBowtie's APPROXIMATE seed mapper, seed_mapper<APPROX_MAPPING> (mapping_inl.h:114-184,288-342): every seed of the stored (reversed) read is
 * searched four times -- forwards in `index` and backwards in `reverse_index` (the FM-index of the REVERSED text, nvBowtie's rfmi), as it
 * stands and complemented -- each search matching its first half exactly and allowing one substitution in the rest; the two searches that
 * start from the seed's near end also report the exact match.  Every non-empty range is pushed to the read's deque under the max_hits
 * rule, in the reference's order, with the reference's flags (position in the read, strand, index direction).  reads_dev: reads of
 * params->read_len symbols back to back (read_bits 2 / 4 / 8).  Deques need nvbio_seed_hits_approx_capacity entries per read. */
nvbio_status nvbio_seed_hits_approx_capacity(uint32_t seeds_per_read, uint32_t seed_len, uint32_t max_hits, uint32_t* capacity);
nvbio_status nvbio_seed_hits_map_approx(nvbio_fm_index_t index, nvbio_fm_index_t reverse_index, const void* reads_dev, uint32_t read_bits,
                                        const uint32_t* read_queue_dev, uint32_t n_reads, const nvbio_seed_hits_params* params,
                                        nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint8_t* reseed_dev, void* stream);

/* select_kernel (select_inl.h:62-130): every active read (active_in_dev[t] = read id | top_flag << 31, the reference's packed_read) whose
 * search has not stopped (trys_dev[read] != 0; NULL = never) and which has a hit left takes a slot of the output queue: its next SA row
 * goes to hits->hit_loc_dev[slot], with hits->hit_read_id_dev[slot], hits->hit_seed_dev[slot] = packed_seed( pos_in_read, index_dir, rc,
 * top_flag ) and active_out_dev[slot]; the row is popped off the front of the read's top (smallest) range in place, an exhausted top
 * range being dropped first (which clears the top flag).  *count_dev = slots written (slot order is arbitrary, as in the reference). */
nvbio_status nvbio_seed_hits_select(int device, const uint32_t* active_in_dev, uint32_t n_active, const uint32_t* trys_dev, uint32_t capacity,
                                    nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint32_t* active_out_dev, const nvbio_hit_queues* hits,
                                    uint32_t* count_dev, void* stream);

/* the tail of nvBowtie's locate kernels (locate_inl.h:127-136,188-198): hit.loc = located position - seed.pos_in_read, uint32 arithmetic,
 * for the hits->n selected hits (positions_dev from nvbio_fm_locate over hits->hit_loc_dev) */
nvbio_status nvbio_seed_hits_loc(int device, const uint32_t* positions_dev, const nvbio_hit_queues* hits, void* stream);

/* score_reduce_kernel with ReduceBestApproxContext (reduce_inl.h:65-140, reduce.h:55-99), one hit per active read: slot i of the scoring
 * queue (hits->hit_score_dev / hit_loc_dev / hit_seed_dev [i]) belongs to read active_dev[i] & 0x7FFFFFFF.
 *   best_dev[4 r ..]  = { a1 score, a1 locus, a2 score, a2 locus } (io::BestAlignments: scores start at the read's worst score, loci at
 *                       0xFFFFFFFF = unaligned, aligner.h:279-301); best_rc_dev[r] = a1 strand | a2 strand << 1
 *   a hit at a locus already held is skipped; a better one becomes a1 (a1 moves to a2); a worse one that beats a2 and is `distinct`
 *   from a1 (other strand or more than read_len / 2 away, nvbio/io/alignments_inl.h:26-38) becomes a2 -- either resets trys_dev[r] to
 *   max_effort; anything else is a failure: from min_ext extensions on (n_ext = extensions before this pass) a hit that is not from
 *   the top seed decrements trys_dev[r], and at zero, or at max_ext extensions, the read's deque is erased (sizes_dev[r] = 0). */
nvbio_status nvbio_score_reduce_effort(int device, const uint32_t* active_dev, const nvbio_hit_queues* hits, uint32_t read_len, uint32_t n_ext,
                                       const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev, uint32_t* trys_dev,
                                       uint32_t* sizes_dev, void* stream);

/* The several-hits-per-read form of the two calls above (select_multi_kernel, select_inl.h:268-437; score_reduce_kernel's loop over a read's
 * hits, reduce_inl.h:94-134): once fewer than half a batch of reads are active nvBowtie takes up to n_multi = BATCH_SIZE / active SA rows per read
 * and pass (aligner_best_approx.h:487-510).  A read's hits take CONSECUTIVE slots of the hit queue in selection order:
 * hits_first_dev[s] / hits_count_dev[s] for the read in slot s of active_out_dev; counts_dev[0] = reads written, counts_dev[1] = hits written
 * (<= n_active * n_multi).  The reduction runs the one-hit rule over every read's hits in that order with n_ext + i as the extension
 * count of hit i (ReduceBestApproxContext::failure( idx, .. ), reduce.h:82-92). */
nvbio_status nvbio_seed_hits_select_multi(int device, const uint32_t* active_in_dev, uint32_t n_active, const uint32_t* trys_dev, uint32_t capacity,
                                          uint32_t n_multi, nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint32_t* active_out_dev,
                                          uint32_t* hits_first_dev, uint32_t* hits_count_dev, const nvbio_hit_queues* hits, uint32_t* counts_dev,
                                          void* stream);
nvbio_status nvbio_score_reduce_effort_multi(int device, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                             const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, uint32_t read_len, uint32_t n_ext,
                                             const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev, uint32_t* trys_dev,
                                             uint32_t* sizes_dev, void* stream);

/* The read queues of nvBowtie's best-approx loop as calls, so that a host loop over this ABI needs no device code of its own
 * (aligner_best_approx.h:77,148-207,363-450):
 *   nvbio_best_approx_init      best_dev[4 r ..] = { worst, -1, worst, -1 }, best_rc_dev[r] = 0: init_alignments( reads, threshold_score )
 *   nvbio_read_queue_begin      for the n reads of queue_dev (NULL: reads 0..n-1), any of: seed_offsets_dev[t] = read * read_len + first_offset (the
 *                               offsets of a seeding pass's seed set), active_dev[t] = read | top_seed << 31 (packed_read), trys_dev[read] =
 *                               max_effort_init (select_init)
 *   nvbio_read_queue_filter     queue_out_dev = the reads of queue_dev (NULL: 0..n-1) with read_flags_dev[read] != 0, in order (the reads that asked
 *                               for reseeding go round again); *count_dev (device) = how many */
nvbio_status nvbio_best_approx_init(int device, uint32_t n_reads, int32_t worst_score, int32_t* best_dev, uint8_t* best_rc_dev, void* stream);
nvbio_status nvbio_read_queue_begin(int device, const uint32_t* queue_dev, uint32_t n, uint32_t read_len, uint32_t first_offset, uint32_t top_seed,
                                    uint32_t max_effort_init, uint32_t* seed_offsets_dev, uint32_t* active_dev, uint32_t* trys_dev, void* stream);
nvbio_status nvbio_read_queue_filter(int device, const uint32_t* queue_dev, uint32_t n, const uint8_t* read_flags_dev, uint32_t* queue_out_dev,
                                     uint32_t* count_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * The same loop over reads of DIFFERENT lengths (a ragged batch: read r = symbols [read_offsets[r], read_offsets[r+1]) of the stored
 * stream).  nvBowtie's map_kernel computes everything per lane (mapping_inl.h:504-529): read_len = range.y - range.x, the filter
 * `read_len < params.min_read_len`, seed_freq( read_len ), retry_stride = seed_freq / (max_reseed + 1), and the walk
 * pos = begin + retry * retry_stride; pos + seed_len <= end; pos += seed_freq.  With M_r the length of read r and L = seed_len:
 *   S_r     = seed_intervals_dev[r]: seed_freq( M_r ), evaluated by the caller as the reference evaluates it (SimpleFunc in float32,
 *             params.h:87-100: int( 1 + 1.15f * sqrtf( M_r ) ) by default)
 *   first_r = seeding_pass * (S_r / (max_reseed + 1))
 *   seed j of read r at stored offset first_r + j * S_r while first_r + j * S_r + L <= M_r: count_r seeds, possibly none
 *   a read with M_r < max( min_read_len, L ) is FILTERED: no seeds in any pass, never flagged for reseeding (:510-514); it ends unaligned.
 *   DIVERGENCE: the reference seeds a read with min_read_len <= M_r < seed_len once, with the whole read (seed_len = min( params.seed_len,
 *   read_len ), :516); this library treats such a read as filtered.
 *   A read that passed the filter but has no seed slot left in this pass (M_r < L + first_r) gets an empty deque, and -- range_count == 0 --
 *   is flagged for reseeding like any read without hits (:549).
 * The arrays of ranges keep ONE stride for the whole batch, seeds_per_read = the largest count_r of the pass (the caller computes it from
 * the lengths); slots count_r .. seeds_per_read-1 of a read are ignored.  M_r < 1024 for every read (SeedHit keeps positions in 10 bits,
 * seed_hit.h:217): the caller checks that, these calls see the lengths on the device only.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    const uint32_t* read_offsets_dev;    /* n_reads + 1 symbol offsets: the batch's sequence_index                               */
    const uint32_t* seed_intervals_dev;  /* n_reads: S_r                                                                         */
    uint32_t        seeds_per_read;      /* stride of the per-seed arrays: the largest number of seeds of a read in this pass    */
    uint32_t        seeding_pass;        /* retry: 0 .. max_reseed                                             (mapping_inl.h:520) */
    uint32_t        max_reseed;
    uint32_t        seed_len;
    uint32_t        min_read_len;        /* params.min_read_len (default 12); the threshold is max( min_read_len, seed_len )      */
} nvbio_ragged_seed_layout;

/* nvbio_read_queue_begin for a ragged batch (mapping_inl.h:504-529 for the offsets; select_init, aligner_best_approx.h:363-450 for the rest):
 * seed_offsets_dev[t * seeds_per_read + j] = read_offsets[read] + first_read + j * S_read for the seeds the read has, 0 for the slots it has
 * not -- a PLAIN string set of n * seeds_per_read strings of seed_len symbols for nvbio_fm_match (offsets_dev = seed_offsets_dev,
 * fixed_len = seed_len, seeds_per_string = 0), since the seed enumeration of nvbio_string_set bases a read's seeds at its first symbol.
 * n_symbols = read_offsets[n_reads] (at least seed_len, so that offset 0 names a string inside the stream). */
nvbio_status nvbio_read_queue_begin_ragged(int device, const uint32_t* queue_dev, uint32_t n, const nvbio_ragged_seed_layout* layout, uint32_t n_symbols,
                                           uint32_t top_seed, uint32_t max_effort_init, uint32_t* seed_offsets_dev, uint32_t* active_dev, uint32_t* trys_dev,
                                           void* stream);
/* nvbio_seed_hits_map for a ragged batch (seed_mapper<EXACT_MAPPING>::enact + map_kernel, mapping_inl.h:193-282,504-556): fw_ranges_dev /
 * rc_ranges_dev [n_reads x seeds_per_read] over the strings of nvbio_read_queue_begin_ragged; the forward hit's pos_in_read is
 * M_r - offset - seed_len (:241); deques need nvbio_seed_hits_capacity( seeds_per_read, max_hits ) entries per read; reseed_dev[r] = 0 for a
 * filtered read, else the rule of :549. */
nvbio_status nvbio_seed_hits_map_ragged(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, const uint32_t* read_queue_dev,
                                        uint32_t n_reads, const nvbio_ragged_seed_layout* layout, uint32_t max_hits, uint32_t rep_seeds,
                                        nvbio_uint2* deques_dev, uint32_t* sizes_dev, uint8_t* reseed_dev, void* stream);
/* init_alignments with every read's own threshold (aligner.h:279-301; min_score( read_len ), aligner_best_approx.h:77):
 * best_dev[4 r ..] = { min_scores_dev[r], -1, min_scores_dev[r], -1 } */
nvbio_status nvbio_best_approx_init_ragged(int device, uint32_t n_reads, const int32_t* min_scores_dev, int32_t* best_dev, uint8_t* best_rc_dev, void* stream);
/* nvbio_score_reduce_effort / _multi with the read's own length in `distinct` (read_len / 2, nvbio/io/alignments_inl.h:26-38; reduce_inl.h:65-140):
 * read_offsets_dev = the n_reads + 1 symbol offsets; of params only max_effort, min_ext and max_ext are read. */
nvbio_status nvbio_score_reduce_effort_ragged(int device, const uint32_t* active_dev, const nvbio_hit_queues* hits, const uint32_t* read_offsets_dev,
                                              uint32_t n_ext, const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev,
                                              uint32_t* trys_dev, uint32_t* sizes_dev, void* stream);
nvbio_status nvbio_score_reduce_effort_multi_ragged(int device, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                                    const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, const uint32_t* read_offsets_dev,
                                                    uint32_t n_ext, const nvbio_seed_hits_params* params, int32_t* best_dev, uint8_t* best_rc_dev,
                                                    uint32_t* trys_dev, uint32_t* sizes_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * nvBowtie's ALL-MAPPING mode (`--mode all`, bowtie2 -a: every placement of a read within max_dist edits), its data-parallel steps
 * (Aligner::all + score_all, nvBowtie/bowtie2/cuda/aligner_all.h:29-139,141-485).  The reference maps ONE seed index per pass
 * (map_exact with seed_range = (seed, seed + 1), aligner_all.h:76-94) through the multi-retry map_kernel (mapping_inl.h:563-634), which,
 * as the reference's code behaves, stores hits at retry == max_reseed only (its other store condition, :627, compares unsigned
 * range_sum < rep_seeds * 0): the seed of pass `seed` sits at stored offset max_reseed * (seed_freq / (max_reseed + 1)) + seed * seed_freq,
 * and a pass whose seed would end past the read has none.  The passes share no state, so the calls below take every seed index at once
 * (or one: seeds_per_read = 1 and first_offset = that seed's offset); the result is the same multiset of alignments.
 *   fw_ranges_dev / rc_ranges_dev [n_reads x seeds_per_read]: the two nvbio_fm_match calls of the exact mapper over the seeds of the
 *   STORED (reversed) reads, exactly as nvbio_seed_hits_map takes them.  Hit order: read-major, then seed index, then the forward
 *   range before the reverse-complemented one, then SA row.  A range counts size & 0xFFFFF rows (SeedHit's 20-bit range_delta,
 *   seed_hit.h:217, as nvbio_seed_hits_map keeps it); there is no max_hits: one seed per pass never fills a deque of max_hits >= 2.
 * Scratch is the caller's: every call that needs some has a *_temp_bytes query and fails with NVBIO_ERR_INVALID on less.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t seeds_per_read;   /* seed slots per read and strand: the stride of the range arrays                                  */
    uint32_t first_offset;     /* stored offset of seed 0: max_reseed * (seed_freq / (max_reseed + 1))        (mapping_inl.h:610) */
    uint32_t seed_interval;    /* seed_freq( read_len )                                                                          */
    uint32_t seed_len;
    uint32_t read_len;         /* reads of one length (< 1024: SeedHit keeps positions in 10 bits)                               */
} nvbio_all_hits_params;

/* gather_ranges + both inclusive_scans of score_all (mapping.cu:29-71, aligner_all.h:209-233) in one scan: slots_dev[2 * n_reads *
 * seeds_per_read] = the inclusive uint64 scan of the range sizes in hit order; a seed that found nothing or holds an N (empty range) and
 * a seed slot that ends past the read (mapping_inl.h:611) contribute 0.  *n_hits_dev (device) = the total.  No host synchronisation. */
nvbio_status nvbio_all_hits_scan_temp_bytes(uint32_t n_reads, uint32_t seeds_per_read, uint64_t* bytes);
nvbio_status nvbio_all_hits_scan(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, uint32_t n_reads,
                                 const nvbio_all_hits_params* params, uint64_t* slots_dev, uint64_t* n_hits_dev, void* temp_dev, uint64_t temp_bytes,
                                 void* stream);

/* select_all_kernel (select.cu:91-135) for the hits [begin, end) of the scan, one lane per hit: hits->hit_loc_dev[o - begin] = the SA
 * row, hits->hit_read_id_dev, hits->hit_seed_dev = packed_seed( pos_in_read, 0, rc, 0 ).  The layout makes read and seed index
 * arithmetic, so the reference's two binary searches (hit -> range -> read) are one.  hits->n = the room of the queues (>= end - begin);
 * a hit past the scan's total is not written. */
nvbio_status nvbio_all_hits_select(int device, const nvbio_uint2* fw_ranges_dev, const nvbio_uint2* rc_ranges_dev, uint32_t n_reads,
                                   const nvbio_all_hits_params* params, const uint64_t* slots_dev, uint64_t begin, uint64_t end,
                                   const nvbio_hit_queues* hits, void* stream);

/* What the reference leaves as a TODO (aligner_all.h:357-358: "sub-sort by read_id/RC flag so as to ... allow removing duplicate
 * extensions"): of the hits->n LOCATED hits (after nvbio_seed_hits_loc) one per distinct (read_id, rc, loc) is kept, in ascending order of
 * (read_id, rc, loc), at the front of hits_out (which may be `hits` itself; dense queues, idx_queue_dev = NULL); *n_out_dev (device) = how
 * many.  The kept hits' packed_seed holds the strand only.  Built on nvbio_sort_unique_keys over key = read_id << 33 | rc << 32 | loc. */
nvbio_status nvbio_all_hits_unique_temp_bytes(uint32_t n, uint64_t* bytes);
nvbio_status nvbio_all_hits_unique(int device, const nvbio_hit_queues* hits, const nvbio_hit_queues* hits_out, uint32_t* n_out_dev, void* temp_dev,
                                   uint64_t temp_bytes, void* stream);

/* AllScoreStream::output for every work item (score_inl.h:671-694): work item i scored hit idx_queue[i] (NULL: hit i) with scores_dev[i];
 * every one with scores_dev[i] >= min_score appends (read_id, rc, loc, score) to the four output arrays from slot out_offset on, IN
 * WORK-ITEM ORDER (the reference hands out ring-buffer slots through an atomic, in arbitrary order).  *count_dev (device) += the
 * number accepted; records that would land at or past out_capacity are dropped, the count is not (the cigar_lens convention). */
nvbio_status nvbio_all_score_output_temp_bytes(uint32_t n, uint64_t* bytes);
nvbio_status nvbio_all_score_output(int device, const nvbio_hit_queues* hits, const int32_t* scores_dev, int32_t min_score, uint32_t* out_read_id_dev,
                                    uint8_t* out_rc_dev, uint32_t* out_loc_dev, int32_t* out_score_dev, uint64_t out_offset, uint64_t out_capacity,
                                    uint64_t* count_dev, void* temp_dev, uint64_t temp_bytes, void* stream);

/* AllTracebackStream::init_context (traceback_inl.h:346-370) for n accepted records: the four per-job arrays of an nvbio_alignment_batch
 * -- read id, the orientation flags nvbio_score_stream_flatten sets (reads_reversed as there), and the window recomputed from the
 * record's locus by the scoring stream's rule -- for nvbio_banded_sw_traceback and nvbio_finish_alignment. */
nvbio_status nvbio_all_traceback_flatten(int device, const uint32_t* rec_read_id_dev, const uint8_t* rec_rc_dev, const uint32_t* rec_loc_dev, uint32_t n,
                                         const uint32_t* read_index_dev, uint32_t band_len, uint32_t genome_len, uint32_t reads_reversed,
                                         uint32_t* read_id_dev, uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * nvBowtie's PAIRED-END best-approx loop, its data-parallel steps (aligner_best_approx_paired.h:84-200,590-1000): the anchor mate's seed hits
 * are walked as in the single-end loop (deques, select, locate: the calls above); a selected hit's anchor is band-aligned against a
 * threshold derived from the best PAIRS found so far (BestAnchorScoreStream, score_inl.h:143-274; compute_target_score,
 * alignment_utils.h:93-102), the hits whose anchor passes get the opposite mate aligned by full-matrix DP in the window the fragment
 * constraints allow (BestOppositeScoreStream, score_inl.h:283-456) and score_reduce_paired_kernel keeps the best two pairs, or the best two
 * alignments of each mate while no pair has been found (reduce_inl.h:157-290).
 * An alignment is 4 int32: { score, position (-1 = none), sink offset, rc | mate << 1 | paired << 2 } (io::Alignment, alignments.h:71-117);
 * best_a_dev / best_o_dev hold two per read pair each (pipeline.best_alignments / best_alignments_o).  Reads of both mates are stored reversed.
 * The sums and differences of score_inl.h:238-239 and :403-413 are uint32, as the reference's.  Where the calls depart from the reference:
 *   - BestAnchorScoreStream::init_context tests `context->min_score > a_optimal_score` before it assigns min_score (score_inl.h:246 vs :249):
 *     the uninitialised term is taken as false;
 *   - an anchor hit that is skipped (its locus is held by one of the four alignments, with the same mate and strand) gets the window (0, 0)
 *     and min_score = INT32_MAX; an anchor hit whose window begins at or past genome_len, or ends before it begins (a locus that wrapped below
 *     zero), gets the window (0, 0) and keeps its min_score;
 *   - an opposite job that cannot run -- min_score above the perfect score, a window that begins at or past genome_len, a locus already held,
 *     begin == end, or end < begin after the uint32 arithmetic -- gets the window (0, 0) with its orientation and min_score as computed;
 *     nvbio_pe_opposite_output takes win_end <= win_begin as "did not run" and reports worst_score, whatever the job's score slot holds,
 *     and loc = win_begin, sink = win_begin + sink.x (a sink.x of 0xFFFFFFFF counts as 0): loc = sink = 0 for a job that
 *     nvbio_pe_opposite_flatten emptied and the scorer left without a sink;
 *   - nvbio_pe_init, like init_alignments, hands `mate` to the constructor argument that is `rc`: best_o starts with rc = 1, mate = 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t anchor;                              /* 0: mate 1 is the anchor of this pass over the batch, 1: mate 2          */
    uint32_t anchor_len, opposite_len;            /* read lengths (uniform)                                                   */
    int32_t  anchor_perfect_score, opposite_perfect_score;   /* scheme.perfect_score( len ) = match * len                    */
    int32_t  anchor_min_score, opposite_min_score;           /* scheme.min_score( len )                                      */
    int32_t  score_limit;                         /* scheme.score_limit(): NVBIO_SCORE_MIN for the Smith-Waterman scheme     */
    int32_t  worst_score;                         /* scheme_type::worst_score = -65536                                       */
    int32_t  match, txt_gap_open, txt_gap_ext;    /* for aln::max_text_gaps (utils_inl.h:145-167)                            */
    uint32_t band, genome_len;
    uint32_t policy, min_frag_len, max_frag_len, overlap, unpaired;   /* NVBIO_PE_POLICY_*, minins, maxins, pe_overlap, pe_unpaired */
    uint32_t max_effort, min_ext, max_ext;
} nvbio_pe_params;
nvbio_status nvbio_pe_init(int device, uint32_t n_reads, int32_t worst_score_mate1, int32_t worst_score_mate2, int32_t* best_a_dev, int32_t* best_o_dev, void* stream);
/* per selected hit: the anchor's banded window + orientation + its min_score (INT32_MAX for a locus already held, whose window is empty) */
nvbio_status nvbio_pe_anchor_flatten(int device, const nvbio_pe_params* params, const nvbio_hit_queues* hits, const int32_t* best_a_dev, const int32_t* best_o_dev,
                                     uint32_t* read_id_dev, uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev,
                                     void* stream);
/* hit.score = score >= min_score ? score : worst_score, hit.sink; hit_opposite_score_dev[i] = worst_score; valid_dev[i] = the anchor passed */
nvbio_status nvbio_pe_anchor_output(int device, const nvbio_pe_params* params, const nvbio_hit_queues* hits, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                    const uint32_t* win_begin_dev, const int32_t* min_scores_dev, int32_t* hit_opposite_score_dev, uint8_t* valid_dev,
                                    void* stream);
/* for the hits queue_dev[0..n) whose anchor passed: the opposite mate's window, orientation and min_score (the empty window where it cannot run) */
nvbio_status nvbio_pe_opposite_flatten(int device, const nvbio_pe_params* params, const uint32_t* queue_dev, uint32_t n, const nvbio_hit_queues* hits,
                                       const int32_t* best_a_dev, const int32_t* best_o_dev, uint32_t* read_id_dev, uint8_t* flags_dev,
                                       uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev, void* stream);
nvbio_status nvbio_pe_opposite_output(int device, const nvbio_pe_params* params, const uint32_t* queue_dev, uint32_t n, const int32_t* scores_dev,
                                      const nvbio_uint2* sinks_dev, const uint32_t* win_begin_dev, const uint32_t* win_end_dev, const int32_t* min_scores_dev,
                                      int32_t* hit_opposite_score_dev, uint32_t* hit_opposite_loc_dev, uint32_t* hit_opposite_sink_dev, void* stream);
/* score_reduce_paired_kernel over every active read's hits (hits_first / hits_count as nvbio_score_reduce_effort_multi) */
nvbio_status nvbio_pe_score_reduce(int device, const nvbio_pe_params* params, const uint32_t* active_dev, uint32_t n_active, const uint32_t* hits_first_dev,
                                   const uint32_t* hits_count_dev, const nvbio_hit_queues* hits, const int32_t* hit_opposite_score_dev,
                                   const uint32_t* hit_opposite_loc_dev, const uint32_t* hit_opposite_sink_dev, uint32_t n_ext, int32_t* best_a_dev,
                                   int32_t* best_o_dev, uint32_t* trys_dev, uint32_t* sizes_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * The same paired loop over mates of DIFFERENT lengths (two ragged batches: mate m of pair r = symbols [offsets_m[r], offsets_m[r+1]) of its
 * stored stream).  The reference's streams are per read throughout: BestAnchorScoreStream and BestOppositeScoreStream take both mates' lengths
 * from each read's own range and evaluate perfect_score( len ) and min_score( len ) per read (score_inl.h:206-213, :341-347), the opposite
 * mate's gap allowance is max_text_gaps( aligner, min_score, o_len ) (:398-399), and score_reduce_paired_kernel's `distinct` distance is
 * read_len / 2 of the ANCHOR read (reduce_inl.h:184-185,240,271); the seeds come from map_kernel, per lane (mapping_inl.h:504-529).  So nothing
 * is approximated: with A_r / O_r the lengths of pair r's anchor / opposite mate,
 *   init              best_a[r] / best_o[r] start from min_scores_mate1_dev[r] / min_scores_mate2_dev[r] (`mate` in the rc slot, as nvbio_pe_init)
 *   anchor flatten    window end begin + band + A_r (clamped); target_pair from a_worst[r] + o_worst[r] while no second pair exists;
 *                     target_mate = max( target_pair - match * O_r, a_worst[r] )
 *   opposite flatten  threshold from o_worst[r]; run = !(min_score > match * O_r); max_text_gaps' loop bounded by O_r; the fragment window from
 *                     A_r and O_r + gaps; policy, min / max fragment, overlap, clamping and the `visited` tests as in the uniform call
 *   reduce            distinct distance A_r / 2 in the paired branch and in the unpaired fallback; everything else as nvbio_pe_score_reduce
 * The ragged calls take nvbio_pe_params -- whose anchor_len, opposite_len and the four perfect / min scores they IGNORE -- and the tables below.
 * min_scores_mate{1,2}_dev[r] = scheme.min_score( length of that mate of pair r ), evaluated by the caller as for nvbio_best_approx_init_ragged;
 * they are given by MATE, the offsets by ROLE: the caller swaps the offsets when the anchor changes, not the min scores.
 * nvbio_pe_anchor_output and nvbio_pe_opposite_output read no length and serve both forms.  The anchor's seeds are those of the single-end
 * ragged loop over the anchor mate's offsets (nvbio_read_queue_begin_ragged, nvbio_seed_hits_map_ragged, with their filter: a mate shorter
 * than max( min_read_len, seed_len ) contributes no seeds while it is the anchor, and is still aligned as the opposite mate of its partner's
 * hits).  Every mate is shorter than 1024 symbols (seed_hit.h:217): the caller checks that, these calls see the lengths on the device only.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    const uint32_t* anchor_offsets_dev;      /* n_reads + 1 symbol offsets of the mate that is the anchor (params->anchor)      */
    const uint32_t* opposite_offsets_dev;    /* n_reads + 1 symbol offsets of the other mate                                    */
    const int32_t*  min_scores_mate1_dev;    /* n_reads: scheme.min_score( len ) of mate 1 of every pair                        */
    const int32_t*  min_scores_mate2_dev;    /* n_reads: the same for mate 2                                                    */
} nvbio_pe_ragged;
/* of `ragged` only the two min-score arrays are read */
nvbio_status nvbio_pe_init_ragged(int device, uint32_t n_reads, const nvbio_pe_ragged* ragged, int32_t* best_a_dev, int32_t* best_o_dev, void* stream);
nvbio_status nvbio_pe_anchor_flatten_ragged(int device, const nvbio_pe_params* params, const nvbio_pe_ragged* ragged, const nvbio_hit_queues* hits,
                                            const int32_t* best_a_dev, const int32_t* best_o_dev, uint32_t* read_id_dev, uint8_t* flags_dev,
                                            uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev, void* stream);
nvbio_status nvbio_pe_opposite_flatten_ragged(int device, const nvbio_pe_params* params, const nvbio_pe_ragged* ragged, const uint32_t* queue_dev, uint32_t n,
                                              const nvbio_hit_queues* hits, const int32_t* best_a_dev, const int32_t* best_o_dev, uint32_t* read_id_dev,
                                              uint8_t* flags_dev, uint32_t* win_begin_dev, uint32_t* win_end_dev, int32_t* min_scores_dev, void* stream);
nvbio_status nvbio_pe_score_reduce_ragged(int device, const nvbio_pe_params* params, const nvbio_pe_ragged* ragged, const uint32_t* active_dev, uint32_t n_active,
                                          const uint32_t* hits_first_dev, const uint32_t* hits_count_dev, const nvbio_hit_queues* hits,
                                          const int32_t* hit_opposite_score_dev, const uint32_t* hit_opposite_loc_dev, const uint32_t* hit_opposite_sink_dev,
                                          uint32_t n_ext, int32_t* best_a_dev, int32_t* best_o_dev, uint32_t* trys_dev, uint32_t* sizes_dev, void* stream);
/* queue_out_dev = the indices i in [0, n) with flags_dev[i] != 0, in order; *count_dev (device) = how many */
nvbio_status nvbio_select_flagged_indices(int device, const uint8_t* flags_dev, uint32_t n, uint32_t* queue_out_dev, uint32_t* count_dev, void* stream);

/* Two conversions a binding of sw-benchmark's stream needs (sw-benchmark/sw-benchmark.cu:70-209): its reference text is packed
 * 2-bit LITTLE-endian (REF_BIG_ENDIAN = false, :64-65; the library reads the big-endian layout of io::SequenceData<DNA>), and its
 * output() stores `sink.score` into an int16 array (:197). */
nvbio_status nvbio_text_2bit_le_to_be(int device, const uint32_t* in_dev, uint32_t n_words, uint32_t* out_dev, void* stream);
nvbio_status nvbio_scores_to_int16(int device, const int32_t* scores_dev, uint32_t n, int16_t* out_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * Gotoh scoring
 * ------------------------------------------------------------------------------------------- */
typedef enum { NVBIO_GLOBAL = 0, NVBIO_LOCAL = 1, NVBIO_SEMI_GLOBAL = 2 } nvbio_alignment_type;   /* alignment.h:242 */

/* The Gotoh scoring-scheme concept (nvbio/alignment/alignment.h:437-449) as data.
 * aln::SimpleGotohScheme(match, mismatch, open, ext) (nvbio/alignment/utils.h:103-123) is
 *   { match, -mismatch, -mismatch, open, ext, open, ext };
 * nvBowtie's SmithWatermanScoringScheme<QualCost,ConstantCost> (nvBowtie/bowtie2/cuda/scoring.h:206-330) is
 *   { m_match, mmp_min, mmp_max, -(read_gap_const+read_gap_coeff), -read_gap_coeff,
 *     -(ref_gap_const+ref_gap_coeff), -ref_gap_coeff }
 * with mismatch(q) = -( mm_min + int( float(min(q,40))/40.0f * (mm_max-mm_min) ) ) (scoring.h:84-88). */
typedef struct
{
    int32_t match;
    int32_t mm_min, mm_max;              /* mismatch penalties (positive) at quality 0 / >= 40 */
    int32_t pat_gap_open, pat_gap_ext;   /* signed scores */
    int32_t txt_gap_open, txt_gap_ext;
} nvbio_gotoh_scheme;

/* The linear-gap Smith-Waterman scheme, aln::SimpleSmithWatermanScheme(match, mismatch, deletion, insertion)
 * (nvbio/alignment/utils.h:81-98), all four as signed scores: `deletion` is charged for a text symbol aligned to no pattern
 * symbol, `insertion` for a pattern symbol aligned to no text symbol (sw/sw_banded_inl.h:369-370,398-431).  The
 * edit-distance aligner is this scheme with (0, -1, -1, -1) (EditDistanceSWScheme, ed/ed_utils.h). */
typedef struct
{
    int32_t match, mismatch, deletion, insertion;
} nvbio_sw_scheme;

#define NVBIO_SCORE_MIN (-(1 << 30))     /* Field_traits<int32>::min(), BestSink's initial score (numbers.h:738-742) */

/* A batch of alignment jobs: the stream concept of aln::Batched[Banded]AlignmentScore
 * (pattern_length / text_length / load_strings; nvbio/alignment/batched.h:274-298, sw-benchmark.cu:70-209,
 * nvBowtie score_inl.h:44-136 + alignment_utils.h:194-308) flattened to arrays.
 *   job i aligns pattern = read[ read_id ? read_id[i] : i ], optionally reversed / complemented
 *   (flags bit0 / bit1: ReadStream, nvbio/io/utils.h:150-168), against text[ win_begin[i], win_end[i] ).   */
typedef struct
{
    const void*     reads_dev;         /* packed big-endian words (read_bits 2, 4) or bytes (8)            */
    uint32_t        read_bits;
    const uint32_t* read_offsets_dev;  /* n_reads+1 symbol offsets (io::SequenceData sequence_index)        */
    const uint8_t*  quals_dev;         /* one byte per read symbol, or NULL (trivial_quality_string -> 0)   */
    const uint32_t* read_id_dev;       /* n entries or NULL                                                 */
    const uint8_t*  flags_dev;         /* n entries or NULL                                                 */
    const void*     text_dev;          /* packed 2-bit big-endian words (text_bits 2) or bytes (8)          */
    uint32_t        text_bits;
    const uint32_t* win_begin_dev;     /* n entries: window begin (symbol index into text)                  */
    const uint32_t* win_end_dev;       /* n entries: window end (exclusive)                                 */
    uint32_t        n;
    uint32_t        max_read_len;      /* the stream's max_pattern_length() (batched.h stream concept), or 0 if
                                          unknown.  It lets the library pick 16-bit packed kernels when every
                                          score provably fits: a job whose pattern is LONGER than a non-zero
                                          max_read_len is rejected (score NVBIO_SCORE_MIN, sink (-1,-1)) rather
                                          than scored in registers that could wrap.                          */
    uint32_t        algo_flags;        /* NVBIO_ALN_*: which of the library's exact shortcuts / kernel variants a
                                          call may use (0 = all; A/B measurements and tests -- results are
                                          identical with every combination)                                  */
    const void*     text_planes_dev;   /* the text as bit planes (nvbio_text_planes_build, or a handle's:
                                          nvbio_fm_index_text_planes), or NULL (what zero-initialising the struct
                                          gives): band-31 end-to-end scoring and its traceback then take a window's
                                          planes with four 16-byte loads from one 128-byte line instead of building
                                          them from 13 packed words per job.  Meaningful with text_bits == 2 only,
                                          128-byte aligned.  The planes describe the text AS IT WAS WHEN THEY WERE
                                          BUILT: pass them only with that very text.  Results are identical.        */
} nvbio_alignment_batch;


enum
{
    NVBIO_ALN_NO_UNGAPPED_SCORE     = 1,   /* every job through the DP (no ungapped end-to-end shortcut, banded and full matrix) */
    NVBIO_ALN_NO_THIRD_CHANCE       = 2,   /* three-mismatch jobs go to the DP                                                  */
    NVBIO_ALN_NO_PACKED_DP          = 4,   /* int32 kernels only                                                                */
    NVBIO_ALN_FORCE_PACKED_DP       = 8,   /* packed full-matrix kernel also for small batches                                  */
    NVBIO_ALN_NO_UNGAPPED_TRACEBACK = 16,  /* every traceback through the direction-vector DP                                   */
    NVBIO_ALN_PK_THREE_WAVES        = 32,  /* packed band-31 kernel built for 3 waves per SIMD (168 VGPRs; the prologue state spills)
                                              instead of 2 (256 VGPRs, nothing spills: the default since the row loop issues without
                                              idle slots and no longer gains from a third wave)                                  */
    NVBIO_ALN_NO_SECOND_CHANCE      = 128, /* two-mismatch jobs go to the DP (A/B: what the check costs inside the first pass)           */
    NVBIO_ALN_NO_NARROW_SCORE       = 512, /* end-to-end full-matrix scoring: every job the shortcut cannot settle through the DP over the whole window
                                              (no band-31 attempt around the best diagonal with its run test)                    */
    NVBIO_ALN_NO_BAND_ROUTE         = 1024, /* full-matrix end-to-end traceback: the jobs whose paths stay within 7 diagonals of their sink keep the
                                              row-restricted full-matrix kernel instead of the band-15 traceback kernel           */
    NVBIO_ALN_PK_STRIPE8            = 256, /* packed full-matrix scoring of end-to-end jobs (match = 0): the general kernel, 8 pattern columns per
                                              stripe, instead of the end-to-end one that sweeps 16 (A/B)                          */
    NVBIO_ALN_RAGGED_READS          = 4096, /* a HINT, the only flag that is not an A/B switch: the batch's reads differ in length.  The packed band-31
                                              end-to-end kernel -- two alignments per lane -- then runs a build that takes a lane's two alignments
                                              in one pass whatever their lengths (the shorter one starts late); without the hint such a lane takes
                                              two passes.  Results are identical either way.                                        */
    NVBIO_ALN_NO_LENGTH_SORT        = 8192, /* with NVBIO_ALN_RAGGED_READS: the DP's job list as it was built instead of in ascending read length (A/B).
                                              Band-31 end-to-end scoring runs first pass -> second chance -> gap (or third) chance -> DP; each kernel appends
                                              the jobs it leaves to the list of the launch that takes them next, so the lists are dense but in no
                                              particular order; no result depends on it.                                              */
    NVBIO_ALN_NO_QUALITY_SHORTCUT   = 2048, /* band-31 end-to-end scoring of reads WITH base qualities under a quality-dependent mismatch penalty
                                              (nvBowtie's default ramp): every job through the DP, as before round 3 (A/B)          */
    NVBIO_ALN_NO_GAP_CHANCE         = 65536, /* band-31 end-to-end scoring: jobs without a near-clean diagonal (reads with an indel) go to the DP instead of the
                                               exact evaluation of their one-gap alignments (gap_chance_e2e31_kernel) (A/B)                               */
    NVBIO_ALN_NO_COOPERATIVE_DP     = 32768, /* full-matrix GLOBAL / SEMI_GLOBAL scoring: one lane per job and the boundary column in memory even where the
                                               several-lanes-per-job kernel (boundary in registers, no scratch) applies (A/B)                           */
    NVBIO_ALN_NO_F16_DP             = 16384, /* packed band-31 DP with 16-bit INTEGER lanes even where the binary16 lanes (exact while every score is an integer of
                                               magnitude <= 2040; one operation less per cell) would do (A/B)                                           */
    NVBIO_ALN_SPLIT_CHANCES         = 131072, /* band-31 end-to-end scoring: the second chance and the gap chance as two launches, one after the other,
                                                instead of one launch with the two roles interleaved (chances_e2e31_kernel) (A/B)                      */
    NVBIO_ALN_NO_PAIRED_GAP_CHANCE  = 262144, /* band-31 end-to-end scoring: the two windows of an indel read (adjacent jobs of one read and strand whose
                                                windows lie 1..5 columns apart) as two gap-chance jobs instead of one that walks their shared
                                                diagonals once (gap_chance_e2e31_pair) (A/B)                                                           */
    NVBIO_ALN_NO_NARROW_DP          = 524288, /* band-31 end-to-end scoring: every DP job over all 31 columns; the first pass forms no classes of jobs whose
                                                score bound U* confines the optimal paths to 13 or 17 columns (banded_gotoh_band31_pk_kernel, NARROW) (A/B) */
    NVBIO_ALN_NO_TEXT_PLANES        = 1048576, /* band-31 end-to-end scoring and traceback: ignore the batch's text_planes_dev and build every window's
                                                 planes from the packed text, as a batch without planes does (A/B)                                     */
    NVBIO_ALN_NO_NARROW_TRACEBACK   = 64   /* band-31 end-to-end traceback: every DP over the whole band (no band-15 route for the jobs
                                              whose optimal paths provably stay within 7 diagonals of the sink)                  */
};

enum { NVBIO_READ_REVERSE = 1, NVBIO_READ_COMPLEMENT = 2 };

/* Best candidate per read after the extension (the per-read score reduction of examples/fmmap/fmmap.cu:367-376, with a
 * total order): for candidate i of read keys_dev[i] >> 34,
 *   sel = max(scores[i] + 2^20, 0) << 34 | strand << 33 | (win_begin[i] + sinks[i].x)     (end position, hit.sink)
 * and best_dev[read] = max(best_dev[read], sel) by 64-bit atomic max.  The caller zero-initialises best_dev;
 * a read without candidates keeps 0.  */
nvbio_status nvbio_best_candidate_reduce(int device, const uint64_t* keys_dev, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                         const uint32_t* win_begin_dev, uint64_t n, uint64_t* best_dev, void* stream);

/* ... and back: scores_dev[r] (NVBIO_SCORE_MIN without a candidate), end_pos_dev[r] (-1 without), rc_dev[r] from best_dev[r].
 * The score field of a selection key is clamped at 0, so every score <= -2^20 unpacks as NVBIO_SCORE_MIN.  That includes the jobs the
 * scorer rejected (score NVBIO_SCORE_MIN, sink 0xFFFFFFFF): a read whose ONLY candidates were rejected has a key that is not 0 and
 * unpacks to score NVBIO_SCORE_MIN, end_pos = win_begin + 0xFFFFFFFF of the candidate with the largest key (no alignment's end: test the
 * score, not end_pos >= 0) and that candidate's strand; nvbio_mapq gives it 0 and nvbio_traceback_best_batch the empty job, as long as
 * min_score > -2^20. */
nvbio_status nvbio_best_candidate_unpack(int device, const uint64_t* best_dev, uint32_t n_reads, int32_t* scores_dev,
                                         int64_t* end_pos_dev, uint8_t* rc_dev, void* stream);

/* The window of every read's best candidate, for the traceback of the best alignments (nvBowtie's banded_traceback_best re-aligns the
 * best alignment inside the window it was scored in, traceback_inl.h:191-247): for every candidate i whose selection key equals
 * best_dev[read] (the final result of nvbio_best_candidate_reduce over ALL candidates),
 *   best_wb_dev[read] = max( best_wb_dev[read], win_begin_dev[i] ),  best_locus_dev[read] = max( ., max( diagonal of keys_dev[i], 0 ) )
 * by 64-bit atomic max (several candidates can tie on the whole key: the largest window begin wins).  The caller initialises both
 * arrays to -1; best_locus_dev may be NULL. */
nvbio_status nvbio_best_candidate_windows(int device, const uint64_t* keys_dev, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                          const uint32_t* win_begin_dev, uint64_t n, const uint64_t* best_dev, int64_t* best_wb_dev,
                                          int64_t* best_locus_dev, void* stream);

/* ... and the traceback batch of all reads from them (one job per read, job r = read r; the stream of banded_traceback_best):
 * flags (strand: NVBIO_READ_REVERSE | NVBIO_READ_COMPLEMENT), window [best_wb, min( best_wb + band + read_len, genome_len )), and
 * the score and sink the scoring pass already found there (sink = (end position - window begin, read_len): for
 * NVBIO_TRACEBACK_SINKS_GIVEN).  A read without a candidate, or whose best score is below min_score, gets the empty window
 * [0, 0), score NVBIO_SCORE_MIN and sink (-1, -1): the traceback reports nothing for it (cigar length 0). */
nvbio_status nvbio_traceback_best_batch(int device, const uint64_t* best_dev, const int64_t* best_wb_dev, uint32_t n_reads, uint32_t read_len,
                                        uint32_t band, uint32_t genome_len, int32_t min_score, uint8_t* flags_dev, uint32_t* win_begin_dev,
                                        uint32_t* win_end_dev, int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream);

/* The second-best alignment per read, as nvBowtie's score_reduce keeps it (nvBowtie/bowtie2/cuda/reduce_inl.h:65-140:
 * best a1 and a second a2 that must be `distinct` from a1 -- io::distinct_alignments, nvbio/io/alignments_inl.h:26-38: the other
 * strand, or more than distinct_dist = read_len / 2 positions away -- and score above the read's threshold; candidates at a
 * location already held are skipped).  The reference's loop depends on the order the extension results arrive in; this is
 * that loop applied to the candidates in descending order of the selection key, in two order-free passes: run
 * nvbio_best_candidate_reduce over ALL candidates first, then this call over the same arrays:
 *   second_dev[read] = max over the read's candidates with scores[i] > worst_score, sel != best_dev[read] and
 *                      distinct( best end position / strand, candidate end position / strand, distinct_dist ) of sel.
 * (Positions are end positions, hit.sink, where the reference compares hit.loc, the diagonal's start: the two differ by
 * read_len +- band.)  The caller zero-initialises second_dev; 0 = no second alignment (BestAlignments::has_second()). */
nvbio_status nvbio_second_candidate_reduce(int device, const uint64_t* keys_dev, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                           const uint32_t* win_begin_dev, uint64_t n, const uint64_t* best_dev,
                                           uint32_t distinct_dist, int32_t worst_score, uint64_t* second_dev, void* stream);

/* Bowtie2's mapping quality of every read from its best and second-best selection keys: BowtieMapq2 (version 2, the
 * evaluator nvBowtie instantiates, bowtie2_cuda_driver.cu:277,600) or BowtieMapq3 (version 3), single-end form of
 * nvBowtie/bowtie2/cuda/mapq.h:32-297.  perfect_score = scheme.perfect_score(read_len) (match * read_len, scoring.h:274),
 * min_score = scheme.min_score(read_len) (MinScoreFunc, scoring.h:117-129), monotone = (match bonus == 0) (scoring.h:339).
 * second_dev may be NULL (no second alignments); second_scores_dev (optional) receives the second-best scores
 * (NVBIO_SCORE_MIN where there is none).  Reads without a candidate get 0. */
typedef struct
{
    int32_t version;         /* 2 or 3 */
    int32_t monotone;
    int32_t perfect_score;
    int32_t min_score;
} nvbio_mapq_params;
nvbio_status nvbio_mapq(int device, const uint64_t* best_dev, const uint64_t* second_dev, uint32_t n_reads,
                        const nvbio_mapq_params* params, int32_t* second_scores_dev, uint8_t* mapq_dev, void* stream);

/* nvbio_best_candidate_reduce + nvbio_best_candidate_unpack + nvbio_second_candidate_reduce + nvbio_mapq in ONE pass over a candidate
 * list that is in TILE ORDER (the per-read score reduction of examples/fmmap/fmmap.cu:367-376 with a total order; nvBowtie's
 * score_reduce, nvBowtie/bowtie2/cuda/reduce_inl.h:65-140, and io::distinct_alignments, nvbio/io/alignments_inl.h:26-38; BowtieMapq2 /
 * BowtieMapq3, nvBowtie/bowtie2/cuda/mapq.h:32-297): the same outputs, bit for bit, with no atomic on device memory, no array
 * the caller has to fill first and every candidate read once.
 * Tile order: candidate i belongs to read keys_dev[i] >> 34; tile t = the reads [t * reads_per_tile, (t + 1) * reads_per_tile), and ALL
 * of their candidates are the entries [tile_offsets_dev[t], tile_offsets_dev[t + 1]) of the list, in any order within the tile
 * (tile_offsets_dev: n_tiles + 1 ascending uint32, [0] = 0, [n_tiles] = n; n_tiles = ceil( n_reads / reads_per_tile ), reads_per_tile
 * <= 192).  That is the order nvbio_fm_match_seed_diagonals_both_tiled leaves its keys in -- tile t's forward keys, then its reverse
 * keys -- as long as nothing was appended behind them (counts_dev[3] == counts_dev[0], no residual keys), and the windows / the extension
 * keep the order of the keys.  A workgroup owns nvbio_finish_reads_tiles_per_group( reads_per_tile ) = 192 / reads_per_tile consecutive
 * tiles and reduces their candidates in LDS.
 * Outputs, every entry of every array written (reads without candidates: key 0 and what the separate calls derive from it):
 *   best_dev / second_dev [n_reads]    the selection keys of nvbio_best_candidate_reduce / nvbio_second_candidate_reduce
 *   scores_out_dev, end_pos_dev, rc_dev  of nvbio_best_candidate_unpack;  mapq_dev, second_scores_dev  of nvbio_mapq
 * distinct_dist, worst_score: as nvbio_second_candidate_reduce; params: as nvbio_mapq.  Ragged reads (read_offsets_dev and
 * min_scores_dev both given): the per-read forms of nvbio_second_candidate_reduce_ragged and nvbio_mapq_ragged( version =
 * params->version, match ); distinct_dist, worst_score and the other fields of params are ignored then.
 * The precondition is checked on the device: offsets that do not ascend from 0 to n, or a candidate whose read is not one of its
 * tile group's, OR 1 into *status_dev (a device word the caller zeroed; it is never cleared here) and that candidate is left out --
 * the caller reads the word once the stream got there and must discard the outputs when it is set.  n = 0 (pointers to the
 * candidates may be NULL) writes every read's no-candidate outputs; n_reads = 0 returns at once. */
nvbio_status nvbio_finish_reads_tiles_per_group(uint32_t reads_per_tile, uint32_t* tiles_per_group);
nvbio_status nvbio_finish_reads(int device, const uint64_t* keys_dev, const int32_t* scores_dev, const nvbio_uint2* sinks_dev,
                                const uint32_t* win_begin_dev, uint64_t n, const uint32_t* tile_offsets_dev, uint32_t n_tiles,
                                uint32_t reads_per_tile, uint32_t n_reads, uint32_t distinct_dist, int32_t worst_score,
                                const nvbio_mapq_params* params, int32_t match, const uint32_t* read_offsets_dev, const int32_t* min_scores_dev,
                                uint64_t* best_dev, uint64_t* second_dev, int32_t* scores_out_dev, int64_t* end_pos_dev, uint8_t* rc_dev,
                                uint8_t* mapq_dev, int32_t* second_scores_dev, uint32_t* status_dev, void* stream);

/* Paired-end: the genome window in which the opposite mate of an anchored mate is aligned (full-matrix DP),
 * BestOppositeScoreStream::init_context (nvBowtie/bowtie2/cuda/score_inl.h:389-425) with frame_opposite_mate
 * (alignment_utils.h:52-88).  g_pos = the anchor hit's locus (hit.loc), anchor_rc its strand, anchor = 0 if mate 1 is
 * the anchor, opposite_gapped_len = opposite mate length + aln::max_text_gaps(aligner, min_score, length)
 * (nvbio/alignment/utils_inl.h:141-162).  flags_dev = how the opposite mate is read (NVBIO_READ_REVERSE |
 * NVBIO_READ_COMPLEMENT when it aligns reverse-complemented); valid_dev = 0 where the window is empty or starts
 * past the genome end (the reference skips such hits). */
enum { NVBIO_PE_POLICY_FF = 0, NVBIO_PE_POLICY_FR = 1, NVBIO_PE_POLICY_RF = 2, NVBIO_PE_POLICY_RR = 3 };
nvbio_status nvbio_opposite_mate_windows(int device, const uint32_t* g_pos_dev, const uint8_t* anchor_rc_dev, uint32_t n,
                                         uint32_t anchor_len, uint32_t opposite_gapped_len, uint32_t anchor, uint32_t policy,
                                         uint32_t min_frag_len, uint32_t max_frag_len, uint32_t overlap, uint32_t genome_len,
                                         uint32_t* win_begin_dev, uint32_t* win_end_dev, uint8_t* flags_dev, uint8_t* valid_dev,
                                         void* stream);

/* Which jobs of a batch the band-31 end-to-end scorer may hand to its gap chance as ONE job (see NVBIO_ALN_NO_PAIRED_GAP_CHANCE):
 * partner_dev[i] = the job paired with job i, or 0xFFFFFFFF.  A function of the batch's geometry alone: jobs j and j + 1 are linked iff they
 * have the same read, the same flags, unclipped windows (win_end - win_begin = read length + 31, read length 1..161) and
 * 0 < |win_begin[j+1] - win_begin[j]| <= NVBIO_GAP_PAIR_MAX_SHIFT (in either order), and j % 64 != 63 (no pair across a wave's 64 jobs); along a run of linked
 * jobs the pairs are taken from its lowest job on ((j, j+1), (j+2, j+3), ...; a job left over stays alone).  The scorer runs a pair as one
 * job only when the first pass sends BOTH to the gap chance and the batch is not declared ragged (NVBIO_ALN_RAGGED_READS); the results never
 * depend on it. */
#define NVBIO_GAP_PAIR_MAX_SHIFT 5
nvbio_status nvbio_banded_gap_pairs(int device, const nvbio_alignment_batch* batch, uint32_t* partner_dev, void* stream);

/* scores_dev[i], sinks_dev[i] = BestSink<int32> (score, (text_end, pattern_end)) after
 * aln::banded_alignment_score<band>( GotohAligner<type>, pattern, quals, text, min_score, sink )
 * (nvbio/alignment/gotoh/gotoh_banded_inl.h:397-688; batched form batched_banded_inl.h:34-157).
 * band must be 3, 7, 15 or 31 (the instantiations nvBowtie dispatches, score_inl.h:468-508).
 * Jobs with text_len < pattern_len report nothing: score NVBIO_SCORE_MIN, sink (-1,-1).       */
nvbio_status nvbio_banded_gotoh_score(int device, uint32_t band, nvbio_alignment_type type,
                                      const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                      int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream);

/* nvbio_banded_gotoh_score plus a report of the route each job took, one byte per job in routes_dev: 0 = settled before the DP (the ungapped
 * shortcut or one of its chances), 1 = the DP over the full band, 2 = the DP's class A (columns 9..21), 3 = its class B (columns 7..23);
 * +8 = a class job whose narrow run could not prove itself exact and which the full band redid.  Scores and sinks never depend on the route;
 * the report exists so that a test can tell which body it exercised. */
nvbio_status nvbio_banded_gotoh_score_routes(int device, uint32_t band, nvbio_alignment_type type,
                                             const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                             int32_t* scores_dev, nvbio_uint2* sinks_dev, uint8_t* routes_dev, void* stream);

/* The same through the reference's staged scheduler: BatchedBandedAlignmentScore<band, stream, DeviceStagedThreadScheduler>
 * (nvbio/alignment/batched_banded_inl.h:165-236; work unit StagedAlignmentUnitBase / BandedScoreUnit, batched_stream.h:117-285),
 * i.e. the windowed banded_alignment_score (banded_inl.h:179-208, gotoh/gotoh_banded_inl.h:703-727) over 32-row windows.  What
 * differs from nvbio_banded_gotoh_score in the RESULT: a job stops at a window's end when max(band) < min_score + rows left x match
 * (:610-622, the sign as the reference has it: exact for a zero match bonus, stricter than "cannot reach min_score" otherwise) -- LOCAL keeps what it reported so far, GLOBAL / SEMI_GLOBAL report nothing (NVBIO_SCORE_MIN, sink (-1,-1)) -- and the
 * band passes through int16 checkpoints clamped at -32736 between windows.  min_score of job i = min_scores_dev[i] (the stream's
 * context->min_score), or min_score for every job when min_scores_dev is NULL.  Instantiated for read_bits/text_bits 4/2, 2/2, 8/8. */
nvbio_status nvbio_banded_gotoh_score_staged(int device, uint32_t band, nvbio_alignment_type type,
                                             const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                             const int32_t* min_scores_dev, int32_t min_score,
                                             int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream);

/* Banded Gotoh traceback: aln::banded_alignment_traceback<band,CHECKPOINTS> / BatchedBandedAlignmentTraceback
 * (nvbio/alignment/banded_inl.h:354-483, gotoh/gotoh_banded_inl.h:730-950; nvBowtie banded_traceback_best,
 * traceback_inl.h:191-247) with nvBowtie's run-length Backtracker as the backtracer
 * (nvBowtie/bowtie2/cuda/alignment_utils.h:115-157).  Per job i:
 *   scores_dev[i], sinks_dev[i]   as nvbio_banded_gotoh_score;
 *   sources_dev[i]                Alignment::source: (text, pattern) cell where the alignment starts;
 *   cigars_dev[i*cigar_stride..]  io::Cigar elements (uint16: type in bits 0-1 -- 0 substitution/match,
 *                                 1 insertion, 2 deletion, 3 soft clip -- length in bits 2-15; nvbio/io/alignments.h:48-66)
 *                                 in BACKTRACKING order, exactly the sequence the Backtracker receives:
 *                                 [clip(pattern_len - sink.y)] ops... [clip(source.y)];
 *   cigar_lens_dev[i]             number of elements produced (elements beyond cigar_stride are dropped, the
 *                                 count is not); 0 with source = sink = (-1,-1) when nothing was reported;
 *                                 0xFFFFFFFF when the pattern is longer than batch->max_read_len (job skipped).
 * batch->max_read_len is REQUIRED here (the stream's max_pattern_length(): it sizes the scratch).
 * The reference recomputes the direction vectors from int16 checkpoints; this call returns
 * NVBIO_ERR_UNSUPPORTED for (scheme, max_read_len) combinations whose scores could leave that range, where the
 * reference's own result is truncation-dependent.
 * flags: NVBIO_TRACEBACK_SINKS_GIVEN -- scores_dev / sinks_dev already hold what nvbio_banded_gotoh_score returns
 * for this very batch (nvBowtie traces alignments it has scored, traceback_inl.h:103-113); the scoring pass is skipped.
 * Implementation note: jobs whose optimum is reached by the diagonal through the sink alone are traced without a
 * DP (the reference's tie rule makes their traceback all substitutions); the others run the DP once, writing
 * their direction vectors to scratch.  Results do not depend on which route a job takes.
 * temp_dev / temp_bytes: optional caller scratch (nvbio_banded_gotoh_traceback_temp_bytes); if NULL the library
 * allocates scratch (kept per stream) and processes the batch in as many launches as 16 GiB allow. */
enum { NVBIO_TRACEBACK_SINKS_GIVEN = 1 };
nvbio_status nvbio_banded_gotoh_traceback_temp_bytes(const nvbio_alignment_batch* batch_host_sizes, uint32_t band, uint64_t* bytes);
nvbio_status nvbio_banded_gotoh_traceback(int device, uint32_t band, nvbio_alignment_type type,
                                          const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                          int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                          uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                          uint32_t flags, void* temp_dev, uint64_t temp_bytes, void* stream);

/* nvbio_banded_gotoh_traceback plus a report of the route each job took, in the manner of nvbio_banded_gotoh_score_routes.  routes_dev, one
 * byte per job: 0 = the ungapped shortcut settled the job, or nothing was traced; 1 = the DP over the full band; 2 = the DP over 15 columns;
 * 3 = the DP over 7 columns (the narrow routes: band 31, SEMI_GLOBAL, match bonus 0, a window of pattern_len + 30 symbols or more, the gap
 * bound drawn from the score at most 7 / 3).  With NVBIO_ALN_NO_UNGAPPED_TRACEBACK every job reaches the DP and reports 1.  band_off_dev,
 * one byte per job: the first column of the job's narrow band for routes 2 and 3, 0 otherwise.  Either pointer may be NULL.  The other
 * outputs never depend on the report; it exists so that a test can tell which kernel body produced a CIGAR. */
nvbio_status nvbio_banded_gotoh_traceback_routes(int device, uint32_t band, nvbio_alignment_type type,
                                                 const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                                 int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                                 uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                                 uint32_t flags, void* temp_dev, uint64_t temp_bytes,
                                                 uint8_t* routes_dev, uint8_t* band_off_dev, void* stream);

/* The same for the linear-gap SmithWatermanAligner (and so for the EditDistanceAligner's scheme (0, -1, -1, -1)):
 * aln::banded_alignment_traceback<band, MAX_PATTERN_LEN, CHECKPOINTS>( SmithWatermanAligner<type>, ... ) (nvbio/alignment/banded_inl.h:354-417
 * over sw/sw_banded_inl.h:281-520 and its walk, :741-797), deletion and insertion costs unequal or not.  As the reference's code behaves,
 * the direction vectors of this aligner carry no SINK (sw_banded_inl.h:420-468): a LOCAL walk does not stop where the score reaches 0
 * but runs on to the first pattern row, so that source.y = 0 for every traced job. */
nvbio_status nvbio_banded_sw_traceback(int device, uint32_t band, nvbio_alignment_type type,
                                       const nvbio_sw_scheme* scheme, const nvbio_alignment_batch* batch,
                                       int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                       uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                       uint32_t flags, void* temp_dev, uint64_t temp_bytes, void* stream);

/* Full-matrix Gotoh traceback: aln::alignment_traceback<..,CHECKPOINTS> / BatchedAlignmentTraceback
 * (nvbio/alignment/alignment_inl.h:355-517, gotoh/gotoh_inl.h:458-538,1573-1640; nvBowtie traceback_best,
 * traceback_inl.h:249-275) with nvBowtie's run-length Backtracker: outputs as nvbio_banded_gotoh_traceback, with
 * x = text and y = pattern coordinates and INSERTION = pattern symbol without text, DELETION = text symbol without
 * pattern.  The scoring is the pattern-blocking pass (the one alignment_traceback itself runs), min_scores_dev
 * (optional) its stripe early exit.  max_pattern_len / max_text_len must bound every job (they size the scratch: a
 * boundary column plus 4 bits per DP cell, for whole waves of 64 jobs: temp_bytes must hold at least 64 jobs); a longer job is
 * skipped and flagged with cigar_lens = 0xFFFFFFFF.
 * flags: NVBIO_TRACEBACK_SINKS_GIVEN as above (scores / sinks from nvbio_full_gotoh_score with text_blocking = 0 and
 * the same min_scores).  NVBIO_ERR_UNSUPPORTED when scores could leave the reference's int16 checkpoints. */
nvbio_status nvbio_full_gotoh_traceback_temp_bytes(const nvbio_alignment_batch* batch_host_sizes, uint32_t max_pattern_len,
                                                   uint32_t max_text_len, uint64_t* bytes);
nvbio_status nvbio_full_gotoh_traceback(int device, nvbio_alignment_type type, const nvbio_gotoh_scheme* scheme,
                                        const nvbio_alignment_batch* batch, uint32_t max_pattern_len, uint32_t max_text_len,
                                        const int32_t* min_scores_dev,
                                        int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                        uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                        uint32_t flags, void* temp_dev, uint64_t temp_bytes, void* stream);

/* nvbio_full_gotoh_traceback plus a report of the route each job took, in the manner of nvbio_banded_gotoh_traceback_routes.  routes_dev, one
 * byte per job: 0 = no DP (nothing to trace, the job was skipped as beyond max_pattern_len / max_text_len, or the diagonal through the sink
 * settled it); 1 = the full matrix over all text rows; 2 = the full matrix over the rows within G diagonals of the sink's; 3 = the band-15
 * kernel over a window of pattern_len + 14 symbols around that diagonal (routes 2 and 3: SEMI_GLOBAL, match bonus 0, the sink in the last
 * pattern row, G = the gap bound drawn from the score at most 250 / 7).  gap_bound_dev, one byte per job: the G the job ran with on routes 2
 * and 3, 0 otherwise.  With NVBIO_ALN_NO_UNGAPPED_TRACEBACK every job reaches the DP over all rows and reports (1, 0).  Neither pointer may
 * be NULL.  The other outputs never depend on the report; it exists so that a test can tell which kernel body produced a CIGAR. */
nvbio_status nvbio_full_gotoh_traceback_routes(int device, nvbio_alignment_type type, const nvbio_gotoh_scheme* scheme,
                                               const nvbio_alignment_batch* batch, uint32_t max_pattern_len, uint32_t max_text_len,
                                               const int32_t* min_scores_dev,
                                               int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                               uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                               uint32_t flags, void* temp_dev, uint64_t temp_bytes,
                                               uint8_t* routes_dev, uint8_t* gap_bound_dev, void* stream);

/* The same for the linear-gap SmithWatermanAligner (and the EditDistanceAligner's scheme (0, -1, -1, -1)), deletion and insertion costs
 * unequal or not: aln::alignment_traceback<MAX_PATTERN_LEN, MAX_TEXT_LEN, CHECKPOINTS>( SmithWatermanAligner<type>, ... )
 * (nvbio/alignment/alignment_inl.h:355-517 over sw/sw_inl.h:306-392 -- the direction of a cell, SINK where a LOCAL score is 0 --,
 * :1476-1600 -- checkpoints and submatrices, swept in stripes of 16 pattern columns -- and its walk, :1644-1694).  Score and sink are
 * those of nvbio_full_sw_score with text_blocking = 0 (run here unless NVBIO_TRACEBACK_SINKS_GIVEN); scratch as
 * nvbio_full_gotoh_traceback_temp_bytes. */
nvbio_status nvbio_full_sw_traceback(int device, nvbio_alignment_type type, const nvbio_sw_scheme* scheme,
                                     const nvbio_alignment_batch* batch, uint32_t max_pattern_len, uint32_t max_text_len,
                                     const int32_t* min_scores_dev,
                                     int32_t* scores_dev, nvbio_uint2* sources_dev, nvbio_uint2* sinks_dev,
                                     uint16_t* cigars_dev, uint32_t cigar_stride, uint32_t* cigar_lens_dev,
                                     uint32_t flags, void* temp_dev, uint64_t temp_bytes, void* stream);

/* nvBowtie finish_alignment (nvBowtie/bowtie2/cuda/traceback_inl.h:536-705) for a batch that has been traced back by
 * either traceback call: from each job's CIGAR (as written by the traceback: backtracking order), its read as aligned and
 * its text window,
 *   ed_dev[i]   = edit distance (mismatches + inserted + deleted symbols; soft clips not counted), the NM of the alignment
 *                 (0 when nothing was traced, 0xFFFFFFFF when the CIGAR had been truncated to cigar_stride);
 *   mds_dev     (optional) = the MDS byte stream nvBowtie keeps per read (nvbio/io/alignments.h:37-43): 2 length bytes, then
 *                 [MDS_MATCH, run <= 255] / [MDS_MISMATCH, read symbol] / [MDS_INSERTION | MDS_DELETION, length, symbols...]
 *                 (soft clips are recorded as insertions, as the reference does); mds_lens_dev[i] = its length (bytes beyond
 *                 mds_stride are dropped, the count is not).
 * sources_dev = Alignment::source of the traceback (source.x = where the alignment starts in the text window). */
nvbio_status nvbio_finish_alignment(int device, const nvbio_alignment_batch* batch, const nvbio_uint2* sources_dev,
                                    const uint16_t* cigars_dev, uint32_t cigar_stride, const uint32_t* cigar_lens_dev,
                                    uint32_t* ed_dev, uint8_t* mds_dev, uint32_t mds_stride, uint32_t* mds_lens_dev, void* stream);

/* full-matrix Gotoh: aln::alignment_score / BatchedAlignmentScore (nvbio/alignment/gotoh/gotoh_inl.h:444-1256,
 * batched_inl.h:39-77).  text_blocking != 0 selects TextBlockingTag (sw-benchmark), 0 the default
 * PatternBlockingTag; min_scores_dev (optional) enables the reference's stripe early exit.
 * temp_dev / temp_bytes: optional caller scratch (see nvbio_full_gotoh_temp_bytes); if NULL the
 * library allocates and frees scratch itself (blocks kept per stream: see "Conventions"). */
nvbio_status nvbio_full_gotoh_temp_bytes(const nvbio_alignment_batch* batch_host_sizes, uint32_t max_pattern_len,
                                         uint32_t max_text_len, int text_blocking, uint64_t* bytes);
nvbio_status nvbio_full_gotoh_score(int device, nvbio_alignment_type type, int text_blocking,
                                    const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                    uint32_t max_pattern_len, uint32_t max_text_len,
                                    const int32_t* min_scores_dev, int32_t* scores_dev, nvbio_uint2* sinks_dev,
                                    void* temp_dev, uint64_t temp_bytes, void* stream);

/* The Myers bit-vector aligner: aln::banded_alignment_score<band>( aln::EditDistanceAligner<TYPE, aln::MyersTag<5> >, ... )
 * (nvbio/alignment/myers/myers_banded_inl.h:172-315), the aligner examples/fmmap/fmmap.cu:346-359 instantiates (SEMI_GLOBAL, band 31).
 * scores_dev[i] = MINUS the edit distance found inside the band that slides down the window's main diagonal, sinks_dev[i] = (text column
 * where it ends, pattern length); NVBIO_SCORE_MIN / (-1,-1) when nothing is reported (text shorter than the pattern, or nothing reaches
 * min_score).  As the reference's code behaves, min_score is truncated to an int16 (:258) -- Field_traits<int32>::min() becomes 0 and
 * only distance-0 columns are reported; pass e.g. -32768 to see every distance.  band <= 32; GLOBAL and SEMI_GLOBAL only; text symbols
 * must be < 4 (the reference's match-vector set leaves the N vector uninitialised). */
nvbio_status nvbio_banded_myers_score(int device, uint32_t band, nvbio_alignment_type type, const nvbio_alignment_batch* batch, int32_t min_score,
                                      int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream);

/* Scoring into aln::Best2Sink<int32>( distinct_dist ) (nvbio/alignment/sink.h:96-116, sink_inl.h:55-83) instead of BestSink: the
 * best alignment in scores_dev / sinks_dev and a second one, ending more than distinct_dist text positions from the first, in
 * scores2_dev / sinks2_dev (NVBIO_SCORE_MIN / (-1,-1) when there is none).  The reference's sink does not demote the old best
 * when a new one arrives, so its result depends on the order of the reports; the kernels report cell by cell in the
 * reference's order (band rows, then columns; 8-wide stripes in the full matrix).  int32 kernels only; reads 2/4/8 bit over
 * 2-bit text, or bytes over bytes. */
nvbio_status nvbio_banded_gotoh_score_best2(int device, uint32_t band, nvbio_alignment_type type,
                                            const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch, uint32_t distinct_dist,
                                            int32_t* scores_dev, nvbio_uint2* sinks_dev, int32_t* scores2_dev, nvbio_uint2* sinks2_dev,
                                            void* stream);
nvbio_status nvbio_full_gotoh_score_best2(int device, nvbio_alignment_type type, int text_blocking,
                                          const nvbio_gotoh_scheme* scheme, const nvbio_alignment_batch* batch,
                                          uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_scores_dev,
                                          uint32_t distinct_dist, int32_t* scores_dev, nvbio_uint2* sinks_dev,
                                          int32_t* scores2_dev, nvbio_uint2* sinks2_dev, void* stream);

/* The other two aligner families of the reference behind the same batch interface:
 * aln::SmithWatermanAligner<TYPE, scheme> and aln::EditDistanceAligner<TYPE> (nvbio/alignment/alignment.h:366-401,508-545).
 *   banded : banded_alignment_score<BAND> -> sw/sw_banded_inl.h:281-520 (the edit-distance aligner runs the same code with
 *            EditDistanceSWScheme, ed/ed_banded_inl.h:37-69: the aligner of examples/fmmap and of nvBowtie --scoring ed);
 *   full   : alignment_score -> sw/sw_inl.h:396-1300, ed/ed_inl.h:60-168.  These two families sweep the matrix in stripes of
 *            16 cells (sw_bandlen_selector, sw/sw_inl.h:1322-1325) where Gotoh uses 8, which decides LOCAL ties and where the
 *            min-score early exit is tested; both are reproduced.
 * Arguments, outputs and scratch exactly as nvbio_banded_gotoh_score / nvbio_full_gotoh_score
 * (nvbio_full_gotoh_temp_bytes sizes the scratch for either).  Qualities are ignored (constant mismatch score). */
nvbio_status nvbio_banded_sw_score(int device, uint32_t band, nvbio_alignment_type type,
                                   const nvbio_sw_scheme* scheme, const nvbio_alignment_batch* batch,
                                   int32_t* scores_dev, nvbio_uint2* sinks_dev, void* stream);
nvbio_status nvbio_full_sw_score(int device, nvbio_alignment_type type, int text_blocking,
                                 const nvbio_sw_scheme* scheme, const nvbio_alignment_batch* batch,
                                 uint32_t max_pattern_len, uint32_t max_text_len,
                                 const int32_t* min_scores_dev, int32_t* scores_dev, nvbio_uint2* sinks_dev,
                                 void* temp_dev, uint64_t temp_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * SAM output: nvBowtie's alignment records as text, formatted on the device (io::SamOutput, nvbio/io/output/output_sam.cpp:76-544, which
 * formats on the host, one fwrite per field and one read after another).  A record is a pure function of arrays the other calls leave
 * in HBM; the text is the reference's byte for byte, with one divergence: generate_md_string sums a run of merged match tokens in a
 * uint8 (a run of 300 prints 44), here the sum has 32 bits.  The header lines (@HD, @PG, @SQ; :155-178) are built on the host
 * (nvbio_amd/sam.hpp sam_header, pipeline.sam_header).
 *   1. nvbio_sam_record_offsets   the byte length of every record and their exclusive uint64 scan (a batch can exceed 4 GiB)
 *   2. the caller reads offsets_dev[n], the total, and allocates the text
 *   3. nvbio_sam_format           writes record i to text_dev[offsets[i], offsets[i + 1])
 * One wave composes one record in LDS and copies it out with 16-byte stores (bytes only at the unaligned head and tail), so a record's
 * text is bounded by the LDS of a wave.  The bound is taken from the declared maxima:
 *   max_name_len + 2 * refs->max_name_len + 2 * max_read_len + 6 * cigar_stride + (2 * mds_stride + 16) + 192   bytes of text,
 *   plus 16 and mds_stride rounded up to 16, must not exceed 16384: else NVBIO_ERR_UNSUPPORTED, before any launch.
 *   The term in brackets bounds the MD text of a well-formed MDS stream (at most 1.5 characters a byte).  A stream that mds_stride cuts,
 *   or that ends, inside a deletion token can print more -- the missing bytes read as 0: up to 255 A's -- and a record that then does not
 *   fit its LDS is refused with NVBIO_SAM_STATUS_TOO_LONG; one that fits is written whole.  The same holds for the BAM calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t        n_seqs;
    uint32_t        max_name_len;         /* the longest sequence name, in bytes                                                          */
    const uint32_t* sequence_index_dev;   /* n_seqs + 1: where each sequence starts in the concatenated genome, [0] = 0
                                             (io::ConstSequenceDataView / bnt.sequence_index, output_sam.cpp:353-356)                     */
    const uint8_t*  names_dev;            /* the sequence names' bytes (bnt.names)                                                        */
    const uint32_t* names_index_dev;      /* n_seqs + 1 offsets into names_dev: name s = [names_index[s], names_index[s + 1]), no NULs     */
} nvbio_sam_refs;

typedef struct
{
    uint32_t        n;                    /* records                                                                                      */
    uint32_t        max_name_len;         /* the longest QNAME, in bytes                                                                  */
    uint32_t        max_read_len;         /* the longest read (< 1024)                                                                    */
    uint32_t        reads_reversed;       /* the reads are stored reversed, as in nvbio_score_stream_flatten (nvBowtie: 1)                */
    const uint8_t*  names_dev;            /* QNAME bytes ...                                                                              */
    const uint32_t* name_index_dev;       /* ... n + 1 offsets into them                                                                  */
    const void*     reads4_dev;           /* the STORED reads, 4-bit big-endian packed words (AlignmentData::read_data, :365-378)         */
    const uint32_t* read_index_dev;       /* n + 1 symbol offsets                                                                         */
    const uint8_t*  quals_dev;            /* one byte per stored symbol, printed + 33 (:382-395); NULL prints `*` (an extension: the
                                             reference always has qualities)                                                               */
    const uint8_t*  state_dev;            /* n: bit 0 aligned, bit 1 rc, bit 2 read 2 (Alignment::mate()), bit 3 paired (is_paired)        */
    const uint32_t* pos_dev;              /* n: cigar_pos, where the alignment starts in the concatenated genome                           */
    const int32_t*  score_dev;            /* n: AS                                                                                        */
    const int32_t*  second_score_dev;     /* n, or NULL: XS; NVBIO_SCORE_MIN = no second alignment, no XS tag (:530-536)                   */
    const uint32_t* ed_dev;               /* n: NM                                                                                        */
    const uint8_t*  mapq_dev;             /* n: MAPQ                                                                                      */
    const uint16_t* cigars_dev;           /* n x cigar_stride, as the traceback calls write them: backtracking order (:188-199)            */
    const uint32_t* cigar_lens_dev;       /* n; a length beyond cigar_stride (0xFFFFFFFF included) is a truncated CIGAR                    */
    const uint8_t*  mds_dev;              /* n x mds_stride, as nvbio_finish_alignment writes them (:216-289), or NULL (MD:Z:*)            */
    const uint32_t* mds_lens_dev;         /* n: the stream's bytes, its two length bytes included; bytes beyond mds_stride are not read   */
    const uint32_t* mate_of_dev;          /* n: the record index of the mate (:437-457,482-519), or NULL: single-end                      */
    uint32_t        cigar_stride;
    uint32_t        mds_stride;
} nvbio_sam_records;

#define NVBIO_SAM_LENGTHS_ONLY 1u       /* nvbio_sam_record_offsets: stop before the scan; offsets_dev[i] = the bytes of record i, [n] = 0      */

/* *status_dev bits of nvbio_sam_format */
#define NVBIO_SAM_STATUS_CAPACITY 1u   /* a record would end past text_capacity: it was not written                                        */
#define NVBIO_SAM_STATUS_OFFSETS  2u   /* offsets_dev is not what nvbio_sam_record_offsets gives for these records: the record was not written */
#define NVBIO_SAM_STATUS_TOO_LONG 4u   /* a record is longer than the declared maxima allow: it was not written                            */

/* the bytes of temp_dev nvbio_sam_record_offsets needs for n records (the scan's; rocPRIM) */
nvbio_status nvbio_sam_format_temp_bytes(uint32_t n, uint64_t* bytes);

/* generate_cigar_string, generate_md_string, process_one_alignment and output_alignment (output_sam.cpp:182-212,216-289,344-544,292-342)
 * as far as they decide a record's LENGTH: offsets_dev[n + 1] = the exclusive uint64 scan of the records' bytes, offsets_dev[n] the total.
 * A record the reference does not write -- an aligned read whose CIGAR was truncated or whose non-D lengths do not sum to the read's
 * length (:474-480) -- takes no bytes.  flags: 0 or NVBIO_SAM_LENGTHS_ONLY (the lengths, not scanned: measurements, or a caller with a scan
 * of its own).  No host synchronisation; n = 0 writes offsets_dev[0] = 0. */
nvbio_status nvbio_sam_record_offsets(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, uint64_t* offsets_dev,
                                      void* temp_dev, uint64_t temp_bytes, void* stream);

/* The same functions for the TEXT (output_sam.cpp:182-544; itoa :76-115; dna_to_char nvbio/basic/dna.h:27-34): record i goes to
 * text_dev[offsets_dev[i], offsets_dev[i + 1]); text_dev must be 16-byte aligned.
 *   not aligned (:419-427,:300-310)  QNAME 4 * 0 0 * * 0 0 SEQ QUAL; the reference's mapq_filter test is inverted and reduces, at its
 *                                    default of -1, to "not aligned": no filter is offered
 *   aligned                          FLAG = 64 | 128 (bit 2), 16 (rc); with a mate 1, 2 (the MATE is paired), 8 (the mate is not aligned), 32 (the mate
 *                                    is rc); RNAME / POS from upper_bound( sequence_index, pos ) - 1; an alignment that ends past its sequence
 *                                    gets 4 ORed in (:459-466) and is then written in the short form above with those flags (:300)
 *   CIGAR                            elements from last to first; RNEXT PNEXT TLEN as :482-524 (a mate whose CIGAR was truncated counts as
 *                                    spanning no reference symbols); tags NM AS [XS] XM XO XG MD in that order (:328-339)
 *   MD, XM, XO, XG                   generate_md_string: merged match runs, a mismatch's symbol, ^ symbols 0 for a deletion, nothing for an
 *                                    insertion; a stream of at most 2 bytes gives MD:Z:* and zero counts
 * *n_skipped_dev (device) = the records that took no bytes.  Checked on the device, in the manner of nvbio_finish_reads: a record that
 * would end past text_capacity, whose offsets are not its own, or that outgrows the declared maxima is not written at all and its
 * NVBIO_SAM_STATUS_* bit is ORed into *status_dev (a device word the caller zeroed; never cleared here).  Nothing is written past
 * min( text_capacity, offsets_dev[n] ). */
nvbio_status nvbio_sam_format(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, const uint64_t* offsets_dev,
                              uint8_t* text_dev, uint64_t text_capacity, uint32_t* n_skipped_dev, uint32_t* status_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * BAM output: the same alignment records in BAM's binary form, and the BGZF container around them, both made on the device
 * (io::BamOutput, nvbio/io/output/output_bam.cpp:65-93,140-225,227-544; BGZF framing nvbio/io/output/output_gzip.cpp:29-42,118-134).
 * The records are a pure function of the nvbio_sam_refs / nvbio_sam_records arrays the SAM calls read, in the same three steps:
 *   1. nvbio_bam_record_offsets   the byte length of every record (its block_size word included) and their exclusive uint64 scan
 *   2. the caller reads offsets_dev[n], the total, and allocates the data (16-byte aligned)
 *   3. nvbio_bam_format           writes record i to data_dev[offsets[i], offsets[i + 1])
 *   4. nvbio_bgzf_frame           wraps any byte string into BGZF blocks: a gzip header, a DEFLATE stream of ONE STORED block
 *                                 (BTYPE 00: uncompressed BAM, what `samtools view -u` writes), CRC-32 and length
 * A file is bam_header (host: nvbio_amd/bam.hpp, pipeline.bam_header) framed on its own, the framed records, and the 28-byte EOF block
 * (:657-659); the caller writes the EOF block.  Compression on the device is not offered: the framing call takes the payload as it is.
 * A group of 16 lanes composes one record in LDS (four records to a wave) and copies it out with 16-byte stores (bytes only at the
 * unaligned head and tail), so a record is bounded by the LDS of a group.  The bound is taken from the declared maxima:
 *   max_name_len + 4 * cigar_stride + max_read_len + (max_read_len + 1) / 2 + (2 * mds_stride + 16) + 72   bytes of record
 *   (36 block_size and fixed fields, the name's NUL, 30 of NM AS XS XM XO XG, 4 of the MD tag's name, type and NUL; an MDS byte of a
 *   well-formed stream prints at most 1.5 characters -- a cut one can print more and ends in NVBIO_BAM_STATUS_TOO_LONG at worst, see the
 *   SAM calls; the term in brackets is 0 without mds_dev), plus 16 and mds_stride rounded up to 16, must not exceed
 *   16384: else NVBIO_ERR_UNSUPPORTED, before any launch.  So are max_name_len > 254 (l_read_name is one byte and counts the NUL) and
 *   cigar_stride > 65535 (n_cigar_op has 16 bits).
 * Divergences from the reference:
 *   1. generate_md_string sums a run of merged match tokens in a uint8; here the sum has 32 bits (as in the SAM calls)
 *   2. next_refID is the mate's sequence index; the reference writes the difference o_seq_index - seq_index (:419), which puts every
 *      mate of a pair on one sequence at refID 0 and is not BAM
 *   3. NVBIO_BAM_REG2BIN is an extension, off by default: the reference leaves bin at 0 (:393-394)
 * ------------------------------------------------------------------------------------------- */
#define NVBIO_BAM_LENGTHS_ONLY 1u       /* nvbio_bam_record_offsets only: stop before the scan; offsets_dev[i] = the bytes of record i, [n] = 0    */
#define NVBIO_BAM_REG2BIN      2u       /* both calls: bin = the SAM specification's reg2bin( pos, pos + reference span ) instead of the reference's 0;
                                           4680 for a record written as unmapped                                                            */

/* *status_dev bits of nvbio_bam_format */
#define NVBIO_BAM_STATUS_CAPACITY 1u   /* a record would end past data_capacity: it was not written                                        */
#define NVBIO_BAM_STATUS_OFFSETS  2u   /* offsets_dev is not what nvbio_bam_record_offsets gives for these records and flags: not written  */
#define NVBIO_BAM_STATUS_TOO_LONG 4u   /* a record is longer than the declared maxima allow: it was not written                            */

/* the bytes of temp_dev nvbio_bam_record_offsets needs for n records (the scan's; rocPRIM) */
nvbio_status nvbio_bam_format_temp_bytes(uint32_t n, uint64_t* bytes);

/* process_one_alignment and output_alignment (output_bam.cpp:227-544) as far as they decide a record's LENGTH: offsets_dev[n + 1] = the
 * exclusive uint64 scan of the records' bytes, offsets_dev[n] the total.  A record the reference does not write -- an aligned read whose
 * CIGAR was truncated or whose non-D lengths do not sum to the read's length (:399-405) -- takes no bytes: exactly the records
 * nvbio_sam_format skips.  flags: NVBIO_BAM_LENGTHS_ONLY, NVBIO_BAM_REG2BIN (which changes no length).  No host synchronisation; n = 0
 * writes offsets_dev[0] = 0. */
nvbio_status nvbio_bam_record_offsets(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, uint64_t* offsets_dev,
                                      void* temp_dev, uint64_t temp_bytes, void* stream);

/* The same functions for the BYTES, little-endian (output_bam.cpp:227-544; generate_cigar :65-93; generate_md_string :140-213; encode_bp
 * :216-225): record i goes to data_dev[offsets_dev[i], offsets_dev[i + 1]); data_dev must be 16-byte aligned.  flags: 0 or NVBIO_BAM_REG2BIN.
 *   framing (:495-544)        block_size (int32: the bytes after it), refID, pos, bin_mq_nl, flag_nc, l_seq, next_refID, next_pos, tlen,
 *                             QNAME + NUL, CIGAR, SEQ, QUAL, tags
 *   not aligned (:330-343)    refID = pos = next_refID = next_pos = -1, tlen = 0, bin_mq_nl = l_read_name alone, flag_nc = 4 << 16 exactly
 *                             (in paired mode too), no CIGAR, no tags
 *   aligned (:346-394)        flags as nvbio_sam_format: 64 | 128 (bit 2), 16 (rc); with a mate 1, 2 (the MATE is paired), 8, 32; refID / pos
 *                             from upper_bound( sequence_index, pos ) - 1, 0-based; bin_mq_nl = l_read_name | mapq << 8, bin 0
 *   ends past its sequence    (:370-385) 4 ORed into the flags, the others kept; the four reference fields -1, tlen 0, n_cigar_op 0, no MAPQ
 *                             (the reference ORs it in later), no tags
 *   CIGAR (:65-93)            elements from last to first, len << 4 | op with M I D S -> 0 1 2 4
 *   SEQ (:254-291)            the orientation nvbio_sam_format prints (both values of reads_reversed); stored symbol s -> 1 << s, any s > 3
 *                             -> 15, complemented first when rc (s < 4 -> 3 - s); high nibble first, the low nibble of an odd tail 0
 *   QUAL (:294-306)           the raw bytes (no + 33), same orientation; quals_dev == NULL writes 0xFF bytes (the BAM specification's
 *                             "absent"; an extension: the reference always has qualities)
 *   mate fields (:407-451)    mate aligned: next_refID its sequence (divergence 2), next_pos 0-based within it, tlen as in SAM (0 across
 *                             sequences, negated when the mate starts first; a mate whose CIGAR was truncated spans no reference symbols);
 *                             mate not aligned: next_refID = refID, next_pos = pos, tlen = 0; single-end: -1, -1, 0
 *   tags (:520-534)           NM c (the low 8 bits of ed), AS i, XS i only with a second score, XM XO XG c (the low 8 bits), MD Z + NUL only
 *                             when the MD string is not empty; string and counts as in nvbio_sam_format (a stream of at most 2 bytes, or
 *                             mds_dev == NULL: empty, zero counts).  The one-byte tag types are the reference's
 * *n_skipped_dev (device) = the records that took no bytes.  Checked on the device: a record that would end past data_capacity, whose
 * offsets are not its own, or that outgrows the declared maxima is not written at all and its NVBIO_BAM_STATUS_* bit is ORed into
 * *status_dev (a device word the caller zeroed; never cleared here).  Nothing is written past min( data_capacity, offsets_dev[n] ).
 * No host synchronisation. */
nvbio_status nvbio_bam_format(int device, const nvbio_sam_refs* refs, const nvbio_sam_records* records, uint32_t flags, const uint64_t* offsets_dev,
                              uint8_t* data_dev, uint64_t data_capacity, uint32_t* n_skipped_dev, uint32_t* status_dev, void* stream);

#define NVBIO_BGZF_BLOCK_BYTES 65280u   /* the payload of a full block (htslib's 0xff00)                                                    */
#define NVBIO_BGZF_OVERHEAD    31u      /* 18 of gzip header + 5 of stored-block header + 8 of trailer                                     */

/* host arithmetic only: *framed_bytes = n_bytes + 31 * ceil( n_bytes / 65280 ) */
nvbio_status nvbio_bgzf_framed_bytes(uint64_t n_bytes, uint64_t* framed_bytes);

/* BGZF framing on the device: block b covers data_dev[65280 b, min( 65280 (b + 1), n_bytes )) and lands at out_dev + 65311 b:
 *   1f 8b 08 04 | mtime 0 (4 bytes) | xfl 00 | os ff | xlen 06 00 | 'B' 'C' 02 00 BSIZE (uint16: the block's bytes - 1)     18 bytes, the gzip
 *                                                                       fields as GzipCompressor sets them (output_gzip.cpp:29-42,118-134)
 *   01 LEN NLEN (uint16 each)                                         one final stored DEFLATE block
 *   the payload
 *   CRC32 (zlib's: polynomial 0xEDB88320, of the payload) ISIZE (uint32 each)
 * One workgroup per block copies the payload with 16-byte loads and stores and computes its CRC-32 in the same pass, with no atomics.
 * data_dev and out_dev must be 16-byte aligned and must not overlap; out_capacity below nvbio_bgzf_framed_bytes( n_bytes ) is refused
 * on the host (NVBIO_ERR_INVALID); nothing is written past the framed bytes.  n_bytes = 0 writes nothing: the EOF block is the caller's.
 * No host synchronisation. */
nvbio_status nvbio_bgzf_frame(int device, const uint8_t* data_dev, uint64_t n_bytes, uint8_t* out_dev, uint64_t out_capacity, void* stream);

/* -------------------------------------------------------------------------------------------
 * FASTQ input: the bytes of a FASTQ file parsed on the device into an io::SequenceData<DNA_N>-shaped batch -- 4-bit big-endian words, a
 * sequence index, one quality byte per symbol, names with a name index: the arrays nvbio_sam_records and the read batches take.  The
 * reference parses on the host one byte at a time (SequenceDataFile_FASTQ_parser::nextChunk, nvbio/io/sequence/sequence_fastq.cpp:39-203)
 * and encodes one read at a time (SequenceDataEncoder::push_back, sequence_encoder.cpp:304-368).
 *
 * The grammar is the reference's: ONE sequential machine over bytes.
 *   state  | '\n'   ' '    '@'    '+'    NUL    0x21..0x7E  other | what the bytes that stay are
 *   GAP    | GAP    GAP    NAME   error  error  error       error | between records; error = the MARKER error, the machine stops (:70-75)
 *   NAME   | SEQ    .      .      .      SEQ    .           .     | the name, '@' '+' ' ' '\r' included (:79-88)
 *   SEQ    | .      .      .      PLUS   PLUS   .           .     | 0x21..0x7E are symbols ('@' too), the rest is dropped: many lines (:103-117)
 *   PLUS   | QUAL   .      .      .      QUAL   .           .     | skipped (:129)
 *   QUAL   | GAP    .      .      .      GAP    .           .     | qualities, '\r' and ' ' included; exactly one line; the record ends (:144-145)
 * The read's length is the QUALITY line's (:143), then min( length, truncate_len ) (sequence_encoder.cpp:315).  Symbols: A a 0, C c 1,
 * G g 2, T t 3, '-' 5, all else 4 (nst_nt4, :30-47); complement bp < 4 ? 3 - bp : 4.  Qualities in uint8 arithmetic: PHRED q, PHRED33
 * q - 33, PHRED64 q - 64, SOLEXA the table (:57-85: 0 1 1 1 1 1 1 2 2 3 3 4 4 5 5 6 7 8 9 10 for q < 20, q - 10 from there).  The
 * strand operator applies to the read after truncation.  End of text in a state other than GAP is the reference's "incomplete read".
 * Departures:
 *   1. qualities are reversed exactly when the symbols are (sequence_string::quality tests the wrong constant, :139: under REVERSE_OP
 *      the reference reverses symbols only, under COMPLEMENT_OP qualities only; every consumer assumes one order)
 *   2. a quality line longer than the kept sequence: the symbols beyond it are 4 (the reference reads stale bytes of the record before)
 *      and NVBIO_FASTQ_STATUS_LENGTH is raised; a shorter one cuts the sequence, as in the reference, and raises the same bit
 *   3. a record with an empty quality line is delivered with length 0 and NVBIO_FASTQ_STATUS_EMPTY (the reference asserts)
 *   4. names are stored without a terminating NUL, with n + 1 offsets, as nvbio_sam_records takes them
 *   5. one strand operator per call (the reference can interleave 2 to 4 copies of each read)
 * Not offered: gzip, FASTA / TXT / SAM / BAM, a CRLF mode (a CRLF file parses as in the reference: into LENGTH errors), max_bps.
 *
 * The machine parallelises as a scan: a byte is a function over the six states (the five and the absorbing error), functions compose
 * associatively.  nvbio_fastq_scan composes 16 bytes per lane, lanes across the wave, waves through LDS, 4096-byte tiles through an
 * array that one workgroup scans -- separate launches, no workgroup waits on another -- then numbers the records' '@' by the record
 * ends before them, and one wave per record finds its fields with ballots.  nvbio_fastq_encode writes the arrays, one wave per record.
 * ------------------------------------------------------------------------------------------- */
#define NVBIO_FASTQ_PHRED   0u
#define NVBIO_FASTQ_PHRED33 1u
#define NVBIO_FASTQ_PHRED64 2u
#define NVBIO_FASTQ_SOLEXA  3u

#define NVBIO_FASTQ_NO_OP                 0u
#define NVBIO_FASTQ_REVERSE_OP            1u
#define NVBIO_FASTQ_COMPLEMENT_OP         2u
#define NVBIO_FASTQ_REVERSE_COMPLEMENT_OP 3u

/* nvbio_fastq_summary.status / *status_dev */
#define NVBIO_FASTQ_STATUS_MARKER     1u   /* a byte other than '\n' ' ' '@' between records: error_offset, error_char; nothing from there on is read */
#define NVBIO_FASTQ_STATUS_INCOMPLETE 2u   /* the text ends inside a record: consumed_bytes = the offset of its '@'                        */
#define NVBIO_FASTQ_STATUS_LENGTH     4u   /* a delivered record's quality line and kept sequence differ in length (departure 2)           */
#define NVBIO_FASTQ_STATUS_EMPTY      8u   /* a delivered record's quality line is empty (departure 3)                                     */
#define NVBIO_FASTQ_STATUS_CAPACITY  16u   /* nvbio_fastq_encode: a record did not fit reads4 / quals / names and was not written          */

typedef struct
{
    uint32_t quality_encoding;   /* NVBIO_FASTQ_PHRED .. NVBIO_FASTQ_SOLEXA (nvBowtie: PHRED33)                                            */
    uint32_t strand_op;          /* NVBIO_FASTQ_NO_OP .. NVBIO_FASTQ_REVERSE_COMPLEMENT_OP (nvBowtie: REVERSE_OP)                          */
    uint32_t truncate_len;       /* reads are cut to this many symbols; 0xFFFFFFFF: never                                                  */
    uint32_t max_records;        /* the machine stops after this many records; 0xFFFFFFFF: never                                           */
} nvbio_fastq_params;

/* what the caller copies back once.  consumed_bytes: text_bytes when the text ends between records; the offset of the unfinished
 * record's '@' (INCOMPLETE); the offset behind the '\n' or NUL that ended record max_records - 1 when max_records stopped the machine
 * (0 for max_records = 0; nothing behind that point is looked at, an error there is not reported); error_offset (MARKER).  A caller
 * that reads a file in chunks puts text[consumed_bytes, text_bytes) in front of the next chunk. */
typedef struct
{
    uint32_t n_records;
    uint32_t consumed_bytes;
    uint32_t n_symbols;          /* read_index[n_records]                                                                                  */
    uint32_t n_name_bytes;       /* name_index[n_records]                                                                                  */
    uint32_t max_read_len;       /* after truncation                                                                                       */
    uint32_t max_name_len;
    uint32_t status;             /* NVBIO_FASTQ_STATUS_*                                                                                   */
    uint32_t error_offset;       /* MARKER: the offending byte's offset and value; else 0xFFFFFFFF and 0                                   */
    uint32_t error_char;
    uint32_t first_bad_record;   /* the first record that raised LENGTH or EMPTY; else 0xFFFFFFFF                                          */
} nvbio_fastq_summary;

/* the bytes of temp_dev both calls need for a text of text_bytes and this max_records: 20 bytes for each of min( max_records,
 * text_bytes / 5 ) records (a record takes 5 bytes at least), 8 for each 4096-byte tile, the record scan's (rocPRIM) */
nvbio_status nvbio_fastq_temp_bytes(uint64_t text_bytes, uint32_t max_records, uint64_t* bytes);

/* The machine over text_dev[0, text_bytes) (16-byte aligned; text_bytes >= 2^32 is NVBIO_ERR_UNSUPPORTED: feed chunks), the records'
 * offsets and lengths, and *summary_dev.  Everything else stays in temp_dev for nvbio_fastq_encode.  No host synchronisation. */
nvbio_status nvbio_fastq_scan(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fastq_params* params, nvbio_fastq_summary* summary_dev,
                              void* temp_dev, uint64_t temp_bytes, void* stream);

/* The arrays of the records nvbio_fastq_scan found, from what it left in temp_dev (same text, text_bytes, params, temp_dev):
 *   reads4_dev      ceil( n_symbols / 8 ) words, symbol i in bits 28 - 4 * (i % 8) of word i / 8; the unused bits of the last word are 0
 *   quals_dev       n_symbols bytes, converted, in the symbols' order; its capacity is that of reads4_dev: 8 * reads4_capacity_words
 *   names_dev       n_name_bytes bytes
 *   read_index_dev, name_index_dev    n_records + 1 offsets each; sized for min( max_records, text_bytes / 5 ) + 1 if the summary was not read
 * A record that would end past a capacity is not written (its index entries are) and NVBIO_FASTQ_STATUS_CAPACITY is ORed into
 * *status_dev (a device word, &summary_dev->status for instance; never cleared here).  Nothing is written past a capacity; upper bounds
 * that fit every record whose lines agree: text_bytes / 2 symbols, text_bytes name bytes (a LENGTH record's quality line may be longer:
 * text_bytes symbols fit always).  No host synchronisation. */
nvbio_status nvbio_fastq_encode(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fastq_params* params, const void* temp_dev,
                                uint64_t temp_bytes, uint32_t* reads4_dev, uint64_t reads4_capacity_words, uint32_t* read_index_dev, uint8_t* quals_dev,
                                uint8_t* names_dev, uint64_t names_capacity, uint32_t* name_index_dev, uint32_t* status_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * FASTA input: the bytes of a reference FASTA file, or of a chunk of one cut anywhere, turned on the device into what the index
 * builder and the SAM writer take -- the 2-bit big-endian packed text nvbio_fm_index_build reads, the sequences' starts and names
 * (nvbio_sam_refs), the holes (runs of ambiguous symbols) and the symbol frequencies.  It is nvBWT's front half, which runs on the host
 * one byte at a time: FASTA_inc_reader::read (nvbio/fasta/fasta_inl.h:64-122) feeding nvBWT's Writer (nvBWT/nvBWT.cu:102-195), whose
 * tables save_bns and save_bpac write as .ann, .amb and .pac (nvbio/basic/bnt.cpp:28-73, nvBWT.cu:243-287).
 *
 * The grammar is the reference's: ONE sequential machine over bytes.
 *   state | '>'    ' '    '\n'   0xFF   other | what the bytes that stay are
 *   PRE   | ID     .      .      END    .     | before the first '>': everything is dropped
 *   ID    | .      REST   BODY   .      .     | the name: every byte up to the first ' ' or '\n', '>' and 0xFF included
 *   REST  | .      .      BODY   .      .     | the rest of the header line, dropped
 *   BODY  | ID     .      .      END    .     | every byte but '\n', ' ', '>' and 0xFF is a symbol: '\r', tab and NUL too.  '>' starts the next
 *         |                                   | sequence anywhere, in mid-line too
 *   END   | .      .      .      .      .     | absorbing: 0xFF is the reader's end-of-file value, tested in PRE and BODY only
 * Symbols: A a 0, C c 1, G g 2, T t 3; every other byte is ambiguous, '-' too (nst_nt4_table gives it 5, the Writer tests c >= 4).  The
 * k-th ambiguous symbol of the whole input, k from 0, is stored as X[k + 1] >> 46 with X[0] = (seed << 16) | 0x330E and
 * X[i + 1] = (0x5DEECE66D * X[i] + 0xB) mod 2^48: uint8( drand48() * 4 ) & 3 after srand48( seed ), seed 11 in nvBWT.
 * A hole (BNTAmb) is a maximal run, within one sequence, of the SAME ambiguous byte among consecutive symbols; line breaks and spaces
 * do not cut it, another byte does ('N' then 'n' are two holes, and so are two 'N' around an 'A').  A sequence (BNTAnnData) has an
 * offset, a length, a name and n_ambs, the holes that start in it.
 * Departures:
 *   a. names are stored without a terminating NUL, with n + 1 offsets, as nvbio_sam_refs takes them
 *   b. input that ends inside a header line raises NVBIO_FASTA_STATUS_INCOMPLETE (the reference's header loops never test for the
 *      end of the file: it does not return)
 *   c. the 1025th, 2049th, ... sequence is kept (nvBWT reads 1024 at a time, and read() has consumed the next record's '>' when it returns)
 *   d. an ambiguous first symbol of a sequence always starts a hole (the Writer compares it with m_lasts = 0: a NUL that comes first
 *      would lengthen the hole before it, or index an empty vector)
 *   e. there is no max_length cut
 *   f. symbol coordinates are 32-bit: an input whose symbols or name bytes would reach 2^32 raises NVBIO_FASTA_STATUS_OVERFLOW_32 and
 *      the chunk that would cross is not encoded
 *   g. a text with no '>' has no sequence (the reference delivers one, nameless and empty)
 * Not offered: gzip, the reversed text (.rpac), .wpac, listing a directory of files: feed them one after another through one state.
 *
 * The machine parallelises as fastq's does: a byte is a function over the five states, functions compose; 16 bytes per lane, lanes
 * across the wave, waves through LDS, 4096-byte tiles through an array that one workgroup scans, in separate launches.  With each
 * tile's entry state known a second pass counts, per tile, symbols, ambiguous symbols, sequence starts, hole starts and name bytes,
 * and takes the tile's first and last symbol byte ("rightmost defined, reset at '>'"); one workgroup scans these.  The body is a
 * stream compaction: nvbio_fasta_encode stages a tile's symbols in LDS in output order, decides hole starts from the staged
 * neighbour (the carried byte for the tile's first symbol), draws an ambiguous symbol by jumping the generator to its global rank
 * (33 affine maps, one per bit of the rank), packs 16 symbols a word and stores whole words, 16 bytes at a time where four words lie
 * inside the tile's range.  The word at either end of a tile's range is shared with its neighbours (or with the chunk before) and is
 * merged with atomicOr into a word that was zeroed.
 * ------------------------------------------------------------------------------------------- */
#define NVBIO_FASTA_PRE  0u
#define NVBIO_FASTA_ID   1u
#define NVBIO_FASTA_REST 2u
#define NVBIO_FASTA_BODY 3u
#define NVBIO_FASTA_END  4u

#define NVBIO_FASTA_NO_SYMBOL 0x100u         /* nvbio_fasta_state.last_symbol: the current sequence has no symbol yet                          */

/* nvbio_fasta_summary.status / *status_dev */
#define NVBIO_FASTA_STATUS_INCOMPLETE  1u   /* the text ends inside a header line (ID or REST): an error only behind the last chunk           */
#define NVBIO_FASTA_STATUS_END_BYTE    2u   /* byte 0xFF in PRE or BODY ended the input (or had ended it before this chunk): consumed_bytes    */
#define NVBIO_FASTA_STATUS_OVERFLOW_32 4u   /* departure f; nvbio_fasta_encode writes nothing and leaves the state as it is                    */
#define NVBIO_FASTA_STATUS_CAPACITY    8u   /* nvbio_fasta_encode: a word, sequence, name byte or hole did not fit and was not written         */

/* The carry from chunk to chunk, 64 bytes in device memory.  nvbio_fasta_state_init sets it, nvbio_fasta_encode advances it, the
 * caller copies it back when it wants the totals.  n_symbols is the text's length so far, freq the counts of the four stored symbols
 * (nvBWT's m_freq: the drawn ones included). */
typedef struct
{
    uint32_t machine;            /* NVBIO_FASTA_PRE .. NVBIO_FASTA_END                                                                     */
    uint32_t n_symbols;
    uint32_t n_seqs;
    uint32_t n_ambs;             /* ambiguous symbols so far = draws so far                                                                */
    uint32_t n_holes;
    uint32_t n_name_bytes;
    uint32_t last_symbol;        /* the last symbol byte of the current sequence, or NVBIO_FASTA_NO_SYMBOL                                 */
    uint32_t seed;
    uint32_t freq[4];
    uint32_t max_name_len;       /* set by nvbio_fasta_finish                                                                              */
    uint32_t reserved[3];
} nvbio_fasta_state;

/* what nvbio_fasta_scan found in ONE chunk, entered in the state it was given.  consumed_bytes is text_bytes, or the offset of the 0xFF
 * that ended the input (0 when an earlier chunk had ended it). */
typedef struct
{
    uint32_t n_symbols;
    uint32_t n_seqs;             /* sequences that START in the chunk                                                                      */
    uint32_t n_ambs;
    uint32_t n_holes;            /* holes that START in the chunk                                                                          */
    uint32_t n_name_bytes;
    uint32_t consumed_bytes;
    uint32_t machine;            /* the state behind the chunk                                                                             */
    uint32_t status;             /* INCOMPLETE, END_BYTE, OVERFLOW_32                                                                      */
} nvbio_fasta_summary;

/* *state_dev = the state in front of the first byte of the first file: PRE, nothing counted, this seed (nvBWT: 11) */
nvbio_status nvbio_fasta_state_init(int device, nvbio_fasta_state* state_dev, uint32_t seed, void* stream);

/* the bytes of temp_dev both calls need for a chunk of text_bytes: 36 for each 4096-byte tile and a header */
nvbio_status nvbio_fasta_temp_bytes(uint64_t text_bytes, uint64_t* bytes);

/* The machine over text_dev[0, text_bytes) (16-byte aligned; text_bytes >= 2^32 is NVBIO_ERR_UNSUPPORTED: feed chunks) entered in
 * *state_dev, which is read and not changed; the tiles' counts stay in temp_dev for nvbio_fasta_encode, *summary_dev is the chunk's
 * totals: what a caller reads to grow its arrays.  No host synchronisation. */
nvbio_status nvbio_fasta_scan(int device, const uint8_t* text_dev, uint64_t text_bytes, const nvbio_fasta_state* state_dev,
                              nvbio_fasta_summary* summary_dev, void* temp_dev, uint64_t temp_bytes, void* stream);

/* The chunk's items, from what nvbio_fasta_scan left in temp_dev (same text, text_bytes and temp_dev, *state_dev as the scan read it),
 * appended at the state's counts; then the state advances by the chunk's counts, whether the items fitted or not:
 *   text2_dev            symbol i in bits 30 - 2 * (i % 16) of word i / 16; text2_capacity_words words, 16-byte aligned.  The words from
 *                        ceil( state.n_symbols / 16 ) on are zeroed first; the word a chunk before filled in part is merged into
 *   seq_offset_dev       [s] = the symbols before sequence s; max_seqs + 1 entries (nvbio_fasta_finish writes entry n_seqs)
 *   name_index_dev       [s] = the name bytes before sequence s; max_seqs + 1 entries
 *   names_dev            names_capacity bytes
 *   hole_offset_dev      [h] = where hole h starts in the text
 *   hole_rank_dev        [h] = the ambiguous symbols before hole h: nvbio_fasta_finish turns the ranks into lengths
 *   hole_amb_dev         [h] = the hole's byte; max_holes entries each
 * An item at or past its capacity is not written and NVBIO_FASTA_STATUS_CAPACITY is ORed into *status_dev (a device word; never cleared
 * here).  Every output pointer may be NULL, which counts as capacity 0 without the bit: with all of them NULL the call only counts
 * (nvBWT's Counter pass) and leaves the same state.  state.freq is counted here, where the draws are made (the counts pass through
 * temp_dev).  Calling it again for the same scan writes the same again.  No host synchronisation. */
nvbio_status nvbio_fasta_encode(int device, const uint8_t* text_dev, uint64_t text_bytes, void* temp_dev, uint64_t temp_bytes,
                                nvbio_fasta_state* state_dev, uint32_t* text2_dev, uint64_t text2_capacity_words, uint32_t* seq_offset_dev,
                                uint32_t* name_index_dev, uint32_t max_seqs, uint8_t* names_dev, uint64_t names_capacity, uint32_t* hole_offset_dev,
                                uint32_t* hole_rank_dev, uint8_t* hole_amb_dev, uint32_t max_holes, uint32_t* status_dev, void* stream);

/* Closes the tables once, behind the last chunk: seq_offset[n_seqs] = n_symbols and name_index[n_seqs] = n_name_bytes (when n_seqs <=
 * max_seqs), hole_len[h] = the ranks' differences (the last from state.n_ambs), seq_n_ambs[s] = the holes that start in sequence s,
 * state.max_name_len.  hole_len_dev and seq_n_ambs_dev may be NULL.  Reads only entries below the capacities and the state's counts. */
nvbio_status nvbio_fasta_finish(int device, nvbio_fasta_state* state_dev, uint32_t* seq_offset_dev, uint32_t* name_index_dev, uint32_t max_seqs,
                                const uint32_t* hole_offset_dev, const uint32_t* hole_rank_dev, uint32_t max_holes, uint32_t* hole_len_dev,
                                uint32_t* seq_n_ambs_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NVBIO_AMD_H */
