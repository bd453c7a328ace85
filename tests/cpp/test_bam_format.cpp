// BAM output from C++ (nvbio_amd/bam.hpp) over the array directory tests/test_gpu_sam_cpp.py::write_arrays writes:
//   bam_format_amd <dir>
// reads <dir>/meta.u32 = { n, n_seqs, max_name_len, ref_max_name_len, max_read_len, reads_reversed, cigar_stride, mds_stride, has_quals,
// has_second_score, has_mds, has_mate_of } and the arrays of nvbio_sam_refs / nvbio_sam_records, one file each, uploads them, formats the
// records through BamFormatter and writes a complete BAM file to stdout: the header's blocks, the records' blocks, the EOF block.  The
// last line goes to stderr: "bam ok: <n> records, <bytes> bytes, <skipped> skipped" (the bytes of the records before framing).
#include <nvbio_amd/nvbio_amd.hpp>
#include <nvbio_amd/bam.hpp>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

template <typename T>
static std::vector<T> load(const std::string& path)
{
    std::ifstream f( path, std::ios::binary );
    std::vector<char> b( (std::istreambuf_iterator<char>( f )), std::istreambuf_iterator<char>() );
    std::vector<T> v( b.size() / sizeof(T) );
    if (!v.empty()) memcpy( v.data(), b.data(), v.size() * sizeof(T) );
    return v;
}

int main(int argc, char** argv)
{
    using namespace nvbio_amd;
    if (argc != 2) { fprintf( stderr, "usage: %s dir\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    try
    {
        const std::vector<uint32_t> meta = load<uint32_t>( dir + "/meta.u32" );
        if (meta.size() != 12) { fprintf( stderr, "meta.u32 does not hold 12 words\n" ); return 1; }
        const std::vector<uint32_t> seq_index = load<uint32_t>( dir + "/seq_index.u32" ), ref_index = load<uint32_t>( dir + "/ref_names_index.u32" );
        const std::vector<uint8_t>  ref_names = load<uint8_t>( dir + "/ref_names.u8" );
        if (seq_index.size() != (size_t)meta[1] + 1u || ref_index.size() != seq_index.size()) { fprintf( stderr, "the sequence tables do not hold n_seqs + 1 entries\n" ); return 1; }

        device_vector<uint32_t> d_seq_index( seq_index ), d_ref_index( ref_index ), d_name_index( load<uint32_t>( dir + "/name_index.u32" ) ),
                                d_reads4( load<uint32_t>( dir + "/reads4.u32" ) ), d_read_index( load<uint32_t>( dir + "/read_index.u32" ) ),
                                d_pos( load<uint32_t>( dir + "/pos.u32" ) ), d_ed( load<uint32_t>( dir + "/ed.u32" ) ),
                                d_cigar_lens( load<uint32_t>( dir + "/cigar_lens.u32" ) ), d_mds_lens( load<uint32_t>( dir + "/mds_lens.u32" ) ),
                                d_mate_of( load<uint32_t>( dir + "/mate_of.u32" ) );
        device_vector<uint8_t>  d_ref_names( ref_names ), d_names( load<uint8_t>( dir + "/names.u8" ) ), d_quals( load<uint8_t>( dir + "/quals.u8" ) ),
                                d_state( load<uint8_t>( dir + "/state.u8" ) ), d_mapq( load<uint8_t>( dir + "/mapq.u8" ) ), d_mds( load<uint8_t>( dir + "/mds.u8" ) );
        device_vector<int32_t>  d_score( load<int32_t>( dir + "/score.i32" ) ), d_second( load<int32_t>( dir + "/second.i32" ) );
        device_vector<uint16_t> d_cigars( load<uint16_t>( dir + "/cigars.u16" ) );

        nvbio_sam_refs refs = nvbio_sam_refs();
        refs.n_seqs = meta[1]; refs.max_name_len = meta[3];
        refs.sequence_index_dev = d_seq_index.data(); refs.names_dev = d_ref_names.data(); refs.names_index_dev = d_ref_index.data();

        nvbio_sam_records rec = nvbio_sam_records();
        rec.n = meta[0]; rec.max_name_len = meta[2]; rec.max_read_len = meta[4]; rec.reads_reversed = meta[5];
        rec.cigar_stride = meta[6]; rec.mds_stride = meta[7];
        rec.names_dev = d_names.data(); rec.name_index_dev = d_name_index.data();
        rec.reads4_dev = d_reads4.data(); rec.read_index_dev = d_read_index.data(); rec.quals_dev = meta[8] ? d_quals.data() : nullptr;
        rec.state_dev = d_state.data(); rec.pos_dev = d_pos.data(); rec.score_dev = d_score.data(); rec.second_score_dev = meta[9] ? d_second.data() : nullptr;
        rec.ed_dev = d_ed.data(); rec.mapq_dev = d_mapq.data(); rec.cigars_dev = d_cigars.data(); rec.cigar_lens_dev = d_cigar_lens.data();
        rec.mds_dev = meta[10] ? d_mds.data() : nullptr; rec.mds_lens_dev = meta[10] ? d_mds_lens.data() : nullptr;
        rec.mate_of_dev = meta[11] ? d_mate_of.data() : nullptr;

        std::vector<std::string> names; std::vector<uint32_t> lengths;
        for (uint32_t s = 0; s < refs.n_seqs; ++s)
        {
            names.push_back( std::string( (const char*)ref_names.data() + ref_index[s], ref_index[s + 1] - ref_index[s] ) );
            lengths.push_back( seq_index[s + 1] - seq_index[s] );
        }
        BamFormatter fmt;
        const std::vector<uint8_t> header = bam_header( names, lengths );
        if (fmt.write_header( stdout, header ) != header.size() + NVBIO_BGZF_OVERHEAD) { fprintf( stderr, "short write\n" ); return 1; }
        fmt.format( refs, rec );
        uint64_t framed = 0;
        check( nvbio_bgzf_framed_bytes( fmt.bytes(), &framed ) );
        if (fmt.write( stdout ) != framed || fmt.write_eof( stdout ) != 28u) { fprintf( stderr, "short write\n" ); return 1; }
        fflush( stdout );
        fprintf( stderr, "bam ok: %u records, %llu bytes, %u skipped\n", rec.n, (unsigned long long)fmt.bytes(), fmt.n_skipped() );
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
    return 0;
}
