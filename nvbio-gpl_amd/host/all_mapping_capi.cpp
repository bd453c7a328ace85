// all_mapping_capi.cpp -- the C++ host loop of host/nvbio_amd/all_mapping.hpp behind one extern "C" entry point (libnvbio_amd_host.so), so that
// Python callers and the parity tests can drive it through ctypes.  Plain g++: no device code; everything on the GPU goes through libnvbio_amd.so.
#include <nvbio_amd/all_mapping.hpp>
#include <nvbio_amd_host.h>

extern "C" {

int nvbio_host_all_mapping(int device, nvbio_fm_index_t fmi, const uint32_t* genome2_dev, uint32_t genome_len, const uint32_t* stored_reads4_dev,
                           uint32_t n_reads, uint32_t read_len, const nvbio_sw_scheme* scheme, int32_t min_score, const nvbio_host_all_mapping_params* p,
                           const nvbio_host_all_mapping_output* out, void* stream, nvbio_host_all_mapping_stats* stats)
{
    try
    {
        nvbio_amd_host::AllMappingParams q;
        q.seed_len = p->seed_len; q.seed_freq = p->seed_freq; q.max_reseed = p->max_reseed; q.max_dist = p->max_dist; q.band = p->band;
        q.aln_type = (nvbio_alignment_type)p->aln_type; q.hits_per_batch = p->hits_per_batch; q.unique = p->unique; q.per_seed_passes = p->per_seed_passes;
        q.want_cigars = p->want_cigars;
        nvbio_amd_host::AllMappingOutput o;
        o.capacity = out->capacity; o.read_id = out->read_id; o.rc = out->rc; o.loc = out->loc; o.score = out->score; o.win_begin = out->win_begin;
        o.source = out->source; o.sink = out->sink; o.ed = out->ed; o.cigars = out->cigars; o.cigar_stride = out->cigar_stride; o.cigar_lens = out->cigar_lens;
        o.mds = out->mds; o.mds_stride = out->mds_stride; o.mds_lens = out->mds_lens;
        const nvbio_amd_host::AllMappingStats s = nvbio_amd_host::all_mapping( device, fmi, genome2_dev, genome_len, stored_reads4_dev, n_reads, read_len, *scheme,
                                                                                min_score, q, o, (hipStream_t)stream );
        if (stats) { stats->n_hits = s.n_hits; stats->n_scored = s.n_scored; stats->n_alignments = s.n_alignments; stats->chunks = s.chunks; stats->pad = 0; }
        return 0;
    }
    catch (const std::exception& e)
    {
        nvbio_host_set_error( e.what() );
        return 1;
    }
}

} // extern "C"
