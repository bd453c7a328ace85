// FASTQ input used from C++ (nvbio_amd/fastq.hpp): reads the FASTQ file at argv[1] through FastqFile in chunks of argv[2] bytes, batches of
// at most argv[3] reads (default 7), and prints every read on one line -- the name's bytes in hex, a tab, the symbols as letters (ACGTN-),
// a tab, the quality bytes in hex -- for tests/test_gpu_fastq_cpp.py to compare with the restatement.  Optional argv[4], argv[5]: the
// strand operator and the quality encoding.  Exit status 0, or 3 when the file ends inside a record (the reads before it are printed).
#include <nvbio_amd/fastq.hpp>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace nvbio_amd;

template <typename T>
static std::vector<T> fetch(const T* dev, size_t n)
{
    std::vector<T> h( n );
    if (n) check_hip( hipMemcpy( h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost ), "hipMemcpy D2H" );
    return h;
}

static void put_hex(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) printf( "%02x", p[i] ); }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf( stderr, "usage: %s reads.fq chunk_bytes [batch_reads [strand_op [quality_encoding]]]\n", argv[0] ); return 2; }
    const size_t   chunk  = (size_t)strtoull( argv[2], nullptr, 10 );
    const uint32_t batch  = argc > 3 ? (uint32_t)strtoul( argv[3], nullptr, 10 ) : 7u;
    const uint32_t strand = argc > 4 ? (uint32_t)strtoul( argv[4], nullptr, 10 ) : NVBIO_FASTQ_NO_OP;
    const uint32_t enc    = argc > 5 ? (uint32_t)strtoul( argv[5], nullptr, 10 ) : NVBIO_FASTQ_PHRED33;
    size_t reads = 0, batches = 0;
    try
    {
        FastqFile file( argv[1], chunk, 0, enc, strand );
        while (file.next_batch( batch ))
        {
            const FastqParser& b = file.batch();
            const nvbio_fastq_summary& s = b.summary();
            const std::vector<uint32_t> words = fetch( b.reads4(), ((size_t)s.n_symbols + 7u) / 8u ), ri = fetch( b.read_index(), (size_t)s.n_records + 1u ),
                                        ni = fetch( b.name_index(), (size_t)s.n_records + 1u );
            const std::vector<uint8_t>  quals = fetch( b.quals(), s.n_symbols ), names = fetch( b.names(), s.n_name_bytes );
            for (uint32_t i = 0; i < s.n_records; ++i)
            {
                put_hex( names.data() + ni[i], ni[i + 1] - ni[i] );
                putchar( '\t' );
                for (uint32_t j = ri[i]; j < ri[i + 1]; ++j) putchar( "ACGTN-??????????"[(words[j >> 3] >> (28u - 4u * (j & 7u))) & 15u] );
                putchar( '\t' );
                put_hex( quals.data() + ri[i], ri[i + 1] - ri[i] );
                putchar( '\n' );
            }
            reads += s.n_records; ++batches;
        }
    }
    catch (const error& e)
    {
        fflush( stdout );
        fprintf( stderr, "%s (after %zu reads)\n", e.what(), reads );
        return std::string( e.what() ).find( "incomplete read" ) != std::string::npos ? 3 : 1;
    }
    fflush( stdout );
    fprintf( stderr, "fastq ok: %zu reads in %zu batches\n", reads, batches );
    return 0;
}
