// FASTA input used from C++ (nvbio_amd/fasta.hpp): reads the FASTA files at argv[2..] through one FastaFile in chunks of argv[1] bytes and
// prints the reference's tables -- a line of totals, one line per sequence (the name's bytes in hex, offset, length, n_ambs), one per hole
// (offset, length, byte) and the FNV-1a hash of the packed text's words -- for tests/test_gpu_fasta_cpp.py to compare with the restatement.
// Exit status 0, or 3 when the input ends inside a header line.
#include <nvbio_amd/fasta.hpp>
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

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf( stderr, "usage: %s chunk_bytes ref.fa [more.fa ...]\n", argv[0] ); return 2; }
    const size_t chunk = (size_t)strtoull( argv[1], nullptr, 10 );
    try
    {
        FastaFile file( nullptr, chunk );
        for (int i = 2; i < argc; ++i) file.read( argv[i] );
        const FastaParser& r = file.finish();
        const nvbio_fasta_state& s = r.state();
        const std::vector<uint32_t> words = fetch( r.text2(), ((size_t)s.n_symbols + 15u) / 16u ), so = fetch( r.seq_offset(), (size_t)s.n_seqs + 1u ),
                                    ni = fetch( r.name_index(), (size_t)s.n_seqs + 1u ), na = fetch( r.seq_n_ambs(), s.n_seqs ),
                                    ho = fetch( r.hole_offset(), s.n_holes ), hl = fetch( r.hole_len(), s.n_holes );
        const std::vector<uint8_t>  names = fetch( r.names(), s.n_name_bytes ), ha = fetch( r.hole_amb(), s.n_holes );
        printf( "total\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", s.n_symbols, s.n_seqs, s.n_holes, s.freq[0], s.freq[1], s.freq[2], s.freq[3], s.max_name_len );
        for (uint32_t i = 0; i < s.n_seqs; ++i)
        {
            printf( "seq\t" );
            for (uint32_t j = ni[i]; j < ni[i + 1]; ++j) printf( "%02x", names[j] );
            printf( "\t%u\t%u\t%u\n", so[i], so[i + 1] - so[i], na[i] );
        }
        for (uint32_t h = 0; h < s.n_holes; ++h) printf( "hole\t%u\t%u\t%u\n", ho[h], hl[h], (unsigned)ha[h] );
        uint64_t hash = 0xcbf29ce484222325ull;
        for (uint32_t w : words)
            for (uint32_t b = 0; b < 4u; ++b) { hash ^= (w >> (8u * b)) & 0xFFu; hash *= 0x100000001b3ull; }
        printf( "text2\t%016llx\n", (unsigned long long)hash );
    }
    catch (const error& e)
    {
        fflush( stdout );
        fprintf( stderr, "%s\n", e.what() );
        return std::string( e.what() ).find( "inside a header line" ) != std::string::npos ? 3 : 1;
    }
    fflush( stdout );
    return 0;
}
