/* nvbio_amd_host.h -- C ABI of libnvbio_amd_host.so: nvBowtie's best-approx and all-mapping loops as C++ host loops over the C ABI of
 * nvbio_amd.h (nvbio-gpl_amd/host/nvbio_amd/best_approx.hpp, all_mapping.hpp), each behind one entry point, so that Python callers, the
 * parity tests and bench.py can drive them through ctypes.  The library holds no device code: everything on the GPU goes through
 * libnvbio_amd.so.
 *
 * Conventions
 *   - every loop returns 0 on success and 1 on failure, and never throws; the message of the last failure on the calling thread is
 *     available from nvbio_host_last_error().
 *   - `*_dev` arguments are device pointers as in nvbio_amd.h; every other array is a HOST array.
 */
#ifndef NVBIO_AMD_HOST_H
#define NVBIO_AMD_HOST_H

#include "nvbio_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* nvbio_host_last_error(void);
void        nvbio_host_set_error(const char* msg);      /* for the library's own entry points */

/* -------------------------------------------------------------------------------------------
 * best-approx (host/nvbio_amd/best_approx.hpp)
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t seed_len, seed_freq, max_hits, rep_seeds, max_effort, max_effort_init, min_ext, max_ext, max_reseed, band, top_seed, batch_size, multi_hit;
} nvbio_host_best_approx_params;
typedef struct { uint64_t n_extensions; uint32_t passes, multi_passes, seeding_passes, pad; } nvbio_host_best_approx_stats;

/* best_dev [4 n_reads] int32 (16-byte aligned), best_rc_dev [n_reads]; n_reads * read_len must stay below 2^32 (returns 1) */
int nvbio_host_best_approx(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                           const uint8_t* quals_dev, uint32_t n_reads, uint32_t read_len, int aln_type, const nvbio_gotoh_scheme* scheme, int32_t worst_score,
                           const nvbio_host_best_approx_params* p, int32_t* best_dev, uint8_t* best_rc_dev, void* stream, nvbio_host_best_approx_stats* stats);

/* the ragged form (best_approx_ragged): read_offsets [n_reads + 1] and min_scores [n_reads] are HOST arrays; a batch holding a read of 1024 symbols or
 * more is refused (returns 1) before anything is launched or written */
int nvbio_host_best_approx_ragged(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                                  const uint8_t* quals_dev, uint32_t n_reads, const uint32_t* read_offsets, int aln_type, const nvbio_gotoh_scheme* scheme,
                                  const int32_t* min_scores, uint32_t min_read_len, const nvbio_host_best_approx_params* p, int32_t* best_dev, uint8_t* best_rc_dev,
                                  void* stream, nvbio_host_best_approx_stats* stats);

typedef struct { uint32_t policy, min_frag_len, max_frag_len, overlap, unpaired; } nvbio_host_paired_params;
typedef struct { uint64_t n_extensions, n_opposite; uint32_t passes, multi_passes; } nvbio_host_paired_stats;

/* the paired-end form: reads1 / reads2 stored reversed, uniform lengths read_len1 / read_len2 (n_reads times either below 2^32); best_a_dev / best_o_dev
 * [n_reads][2][4] int32 */
int nvbio_host_best_approx_paired(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads1_dev,
                                  const uint32_t* stored_reads2_dev, const uint8_t* quals1_dev, const uint8_t* quals2_dev, uint32_t n_reads, uint32_t read_len1,
                                  uint32_t read_len2, int aln_type, const nvbio_gotoh_scheme* scheme, int32_t worst_score1, int32_t worst_score2,
                                  const nvbio_host_best_approx_params* p, const nvbio_host_paired_params* pe, int32_t* best_a_dev, int32_t* best_o_dev, void* stream,
                                  nvbio_host_paired_stats* stats);

/* the paired-end form over mates of different lengths (best_approx_paired_ragged): read_offsets1 / read_offsets2 [n_reads + 1] and min_scores1 / min_scores2
 * [n_reads] are HOST arrays; a missing table, decreasing offsets, an empty mate or a mate of 1024 symbols or more in either batch is refused (returns 1)
 * before anything is launched or written */
int nvbio_host_best_approx_paired_ragged(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads1_dev,
                                         const uint32_t* stored_reads2_dev, const uint8_t* quals1_dev, const uint8_t* quals2_dev, uint32_t n_reads,
                                         const uint32_t* read_offsets1, const uint32_t* read_offsets2, int aln_type, const nvbio_gotoh_scheme* scheme,
                                         const int32_t* min_scores1, const int32_t* min_scores2, uint32_t min_read_len, const nvbio_host_best_approx_params* p,
                                         const nvbio_host_paired_params* pe, int32_t* best_a_dev, int32_t* best_o_dev, void* stream, nvbio_host_paired_stats* stats);

/* -------------------------------------------------------------------------------------------
 * all-mapping (host/nvbio_amd/all_mapping.hpp)
 * ------------------------------------------------------------------------------------------- */
typedef struct
{
    uint32_t seed_len, seed_freq, max_reseed, max_dist, band, aln_type, hits_per_batch, unique, per_seed_passes, want_cigars;
} nvbio_host_all_mapping_params;
/* device arrays of `capacity` records; the ones from win_begin on are read with want_cigars only (mds / mds_lens may be NULL) */
typedef struct
{
    uint64_t     capacity;
    uint32_t*    read_id; uint8_t* rc; uint32_t* loc; int32_t* score;
    uint32_t*    win_begin; nvbio_uint2* source; nvbio_uint2* sink; uint32_t* ed; uint16_t* cigars; uint32_t* cigar_lens; uint8_t* mds; uint32_t* mds_lens;
    uint32_t     cigar_stride, mds_stride;
} nvbio_host_all_mapping_output;
typedef struct { uint64_t n_hits, n_scored, n_alignments; uint32_t chunks, pad; } nvbio_host_all_mapping_stats;

/* stats->n_alignments may exceed out->capacity (the records past it are dropped) */
int nvbio_host_all_mapping(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                           uint32_t n_reads, uint32_t read_len, const nvbio_sw_scheme* scheme, int32_t min_score, const nvbio_host_all_mapping_params* p,
                           const nvbio_host_all_mapping_output* out, void* stream, nvbio_host_all_mapping_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* NVBIO_AMD_HOST_H */
