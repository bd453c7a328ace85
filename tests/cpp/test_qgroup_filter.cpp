// The C++ mirror QGroupIndexDevice / QGroupSetIndexDevice under QGramFilterDevice (nvbio_amd.hpp) over files written by
// tests/test_gpu_qgroup_cpp.py:
//   test_qgroup_filter <dir> <q> <seed_interval> <merge_interval>
// reads <dir>/text.u8 (symbols 0..3), <dir>/reads.u8 (concatenated, 8-bit, N = 4) and <dir>/offsets.u32 (n + 1).  It streams the
// text's q-grams (generate_qgrams, sorted) through a filter over a q-group index of the text and one over a q-group set index of
// the reads, and writes, per index kind k in {string, set}: <k>_ranges.u32, <k>_slots.u64, <k>_hits.u32, <k>_merged.u32,
// <k>_counts.u32 and <k>_ss.u32 (the index's SS through its view).
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
static void save(const std::string& path, const T* p, size_t bytes)
{
    std::ofstream f( path, std::ios::binary );
    f.write( (const char*)p, bytes );
}
template <typename T>
static std::vector<T> fetch(const T* dev, size_t n)
{
    std::vector<T> h( n );
    if (n) nvbio_amd::check_hip( hipMemcpy( h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost ), "fetch" );
    return h;
}

// rank, locate and merge the queries through a filter over `index`; write the outputs under <dir>/<kind>_*
template <typename index_type>
static void run(const std::string& dir, const char* kind, const index_type& index, const nvbio_amd::device_vector<uint64_t>& qgrams,
                const nvbio_amd::device_vector<uint32_t>& positions, uint32_t merge_interval)
{
    using namespace nvbio_amd;
    typedef typename index_type::hit_type      hit_type;
    typedef typename index_type::diagonal_type diagonal_type;
    QGramFilterDevice<index_type> filter;
    const uint32_t n = (uint32_t)qgrams.size();
    const uint64_t n_hits = filter.rank( index, n, qgrams.data(), positions.data() );
    device_vector<hit_type> hits( n_hits );
    filter.locate( 0, n_hits, hits.data() );
    device_vector<diagonal_type> merged( n_hits );
    device_vector<uint32_t>      counts( n_hits );
    const uint32_t n_merged = filter.merge( merge_interval, (uint32_t)n_hits, hits.data(), merged.data(), counts.data() );
    check_hip( hipDeviceSynchronize(), "run" );
    const std::string p = dir + "/" + kind;
    const std::vector<nvbio_uint2> r = fetch( filter.ranges(), n );
    const std::vector<uint64_t>    s = fetch( filter.slots(), n );
    const std::vector<hit_type>    h = hits.to_host();
    const std::vector<diagonal_type> m = fetch( merged.data(), n_merged );
    const std::vector<uint32_t>    c = fetch( counts.data(), n_merged );
    save( p + "_ranges.u32", r.data(), r.size() * sizeof(nvbio_uint2) );
    save( p + "_slots.u64", s.data(), s.size() * 8u );
    save( p + "_hits.u32", h.data(), h.size() * sizeof(hit_type) );
    save( p + "_merged.u32", m.data(), m.size() * sizeof(diagonal_type) );
    save( p + "_counts.u32", c.data(), c.size() * 4u );
    const std::vector<uint32_t> ss = fetch( index.SS(), (size_t)index.n_unique_qgrams() + 1u );
    save( p + "_ss.u32", ss.data(), ss.size() * 4u );
    printf( "%s: %llu hits, %u merged\n", kind, (unsigned long long)n_hits, n_merged );
}

int main(int argc, char** argv)
{
    using namespace nvbio_amd;
    if (argc != 5) { fprintf( stderr, "usage: %s dir q seed_interval merge_interval\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    const uint32_t q = (uint32_t)strtoul( argv[2], 0, 0 );
    const uint32_t seed_interval = (uint32_t)strtoul( argv[3], 0, 0 ), merge_interval = (uint32_t)strtoul( argv[4], 0, 0 );
    try
    {
        std::vector<uint8_t>        text    = load<uint8_t>( dir + "/text.u8" );
        std::vector<uint8_t>        reads   = load<uint8_t>( dir + "/reads.u8" );
        const std::vector<uint32_t> offsets = load<uint32_t>( dir + "/offsets.u32" );
        const uint32_t text_len = (uint32_t)text.size();
        text.resize( text.size() + 16, 0 ); reads.resize( reads.size() + 16, 0 );
        device_vector<uint8_t>  d_text( text ), d_reads( reads );
        device_vector<uint32_t> d_offs( offsets );
        const string_set set = string_set::concatenated( d_reads.data(), 8u, d_offs.data(), (uint32_t)offsets.size() - 1u );

        QGroupIndexDevice text_index;
        text_index.build( q, 2u, text_len, d_text.data(), 8u );
        QGroupSetIndexDevice read_index;
        read_index.build( q, 2u, set, seed_interval );
        if (text_index.n_qgrams() != text_len || text_index.n_words() != (1ull << (2u * q)) / 32u + 1u || text_index.slots() != text_index.SS() ||
            text_index.qgrams() != nullptr || read_index.table() == nullptr)
        {
            fprintf( stderr, "view mismatch\n" ); return 1;
        }

        device_vector<uint64_t> qgrams( text_len );
        device_vector<uint32_t> positions( text_len );
        generate_qgrams( 0, q, 2u, d_text.data(), 8u, text_len, 0u, text_len, qgrams.data(), positions.data(), true );
        run( dir, "string", text_index, qgrams, positions, merge_interval );
        run( dir, "set", read_index, qgrams, positions, merge_interval );
        printf( "qgroup filter ok\n" );
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
    return 0;
}
