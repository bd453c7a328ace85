// The C++ mirror of the sufsort module (nvbio_amd.hpp, namespace cuda) over files written by tests/test_gpu_sufsort_cpp.py:
//   test_sufsort <dir> <bits> <flags>
// reads <dir>/symbols.bin (the packed set: 2- or 4-bit big-endian words, or bytes), <dir>/offsets.u32 (n + 1) and <dir>/text2.u32
// with <dir>/text_len.u32 (a 2-bit packed text).  The handlers write what they receive: sort_global.u32, sort_ids.u32, sort_cum.u32
// (cuda::suffix_sort of the set), bwt_host.u8, bwt_dev.u8, suf_host.u32, suf_dev.u32 (cuda::bwt of the set), and sa.u32, bwt.u32,
// primary.u32 (the single-string entries).
#include <nvbio_amd/nvbio_amd.hpp>
#include <cstdio>
#include <cstdlib>
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
template <typename T>
static void save(const std::string& path, const T* p, size_t count)
{
    std::ofstream f( path, std::ios::binary );
    f.write( (const char*)p, count * sizeof(T) );
}
template <typename T>
static std::vector<T> fetch(const T* dev, size_t n)
{
    std::vector<T> h( n );
    if (n) nvbio_amd::check_hip( hipMemcpy( h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost ), "fetch" );
    return h;
}

struct SortHandler
{
    std::string dir; uint32_t n_strings; uint32_t n;
    void process(const uint32_t n_suffixes, const uint32_t* suffix_array, const uint32_t* string_ids, const uint32_t* cum_lengths)
    {
        n = n_suffixes;
        save( dir + "/sort_global.u32", fetch( suffix_array, n ).data(), n );
        save( dir + "/sort_ids.u32", fetch( string_ids, n ).data(), n );
        save( dir + "/sort_cum.u32", fetch( cum_lengths, n_strings ).data(), n_strings );
    }
};

struct BWTHandler
{
    std::string dir; uint32_t n;
    void process(const uint32_t n_suffixes, const uint8_t* h_bwt, const uint8_t* d_bwt, const nvbio_uint2* h_suffixes, const nvbio_uint2* d_suffixes,
                 const uint32_t* d_indices)
    {
        n = n_suffixes;
        if (d_indices != nullptr) throw std::runtime_error( "d_indices is not NULL" );
        save( dir + "/bwt_host.u8", h_bwt, n );
        save( dir + "/bwt_dev.u8", fetch( d_bwt, n ).data(), n );
        save( dir + "/suf_host.u32", h_suffixes, n );
        save( dir + "/suf_dev.u32", fetch( d_suffixes, n ).data(), n );
    }
};

int main(int argc, char** argv)
{
    using namespace nvbio_amd;
    if (argc != 4) { fprintf( stderr, "usage: %s dir bits flags\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    const uint32_t bits = (uint32_t)strtoul( argv[2], 0, 0 ), flags = (uint32_t)strtoul( argv[3], 0, 0 );
    try
    {
        const std::vector<uint8_t>  symbols = load<uint8_t>( dir + "/symbols.bin" );
        const std::vector<uint32_t> offsets = load<uint32_t>( dir + "/offsets.u32" );
        device_vector<uint8_t>  d_symbols( symbols );
        device_vector<uint32_t> d_offs( offsets );
        const string_set set = string_set::concatenated( d_symbols.data(), bits, d_offs.data(), (uint32_t)offsets.size() - 1u );

        nvbio_sufsort_stats stats;
        SortHandler sort_handler{ dir, set.size(), 0u };
        cuda::suffix_sort( set, sort_handler, flags, 0, 0, &stats );
        BWTHandler bwt_handler{ dir, 0u };
        cuda::bwt( set, bwt_handler, flags );
        if (sort_handler.n != bwt_handler.n || stats.n_suffixes != sort_handler.n || stats.rounds == 0) { fprintf( stderr, "count mismatch\n" ); return 1; }

        const std::vector<uint32_t> text2 = load<uint32_t>( dir + "/text2.u32" );
        const uint32_t text_len = load<uint32_t>( dir + "/text_len.u32" )[0];
        device_vector<uint32_t> d_text( text2 ), sa( (size_t)text_len + 1u ), words( ((size_t)text_len + 15u) / 16u );
        cuda::suffix_sort( text_len, d_text.data(), sa.data() );
        const uint32_t primary = cuda::bwt( text_len, d_text.data(), words.data() );
        if (primary != cuda::find_primary( text_len, d_text.data() )) { fprintf( stderr, "primary mismatch\n" ); return 1; }
        save( dir + "/sa.u32", sa.to_host().data(), sa.size() );
        save( dir + "/bwt.u32", words.to_host().data(), words.size() );
        save( dir + "/primary.u32", &primary, 1 );
        printf( "sufsort ok: %u suffixes, %u rounds\n", stats.n_suffixes, stats.rounds );
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
    return 0;
}
