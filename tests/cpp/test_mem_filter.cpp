// The C++ mirror MEMFilter<amd_device_tag> (nvbio_amd.hpp) over files written by tests/test_gpu_mem_cpp.py:
//   test_mem_filter <dir> <min_intv> <max_intv> <min_span> <split_len> <split_width>
// reads <dir>/text.u8 (symbols 0..3), <dir>/reads.u8 (concatenated, 8-bit, N = 4) and <dir>/offsets.u32 (n + 1), builds the forward
// and reverse indices on the GPU, runs rank and locate, and writes ranges.u32 (n_ranges x 4), first.u32, slots.u64 and hits.u32.
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
static void save(const std::string& path, const std::vector<T>& v)
{
    std::ofstream f( path, std::ios::binary );
    f.write( (const char*)v.data(), v.size() * sizeof(T) );
}
// big-endian 2-bit packing (PackedStream<uint32,2,true>), with padding words
static std::vector<uint32_t> pack2(const std::vector<uint8_t>& s)
{
    std::vector<uint32_t> w( (s.size() + 15) / 16 + 4, 0u );
    for (size_t i = 0; i < s.size(); ++i) w[i >> 4] |= (uint32_t)(s[i] & 3u) << (30u - 2u * (i & 15u));
    return w;
}

int main(int argc, char** argv)
{
    using namespace nvbio_amd;
    if (argc != 7) { fprintf( stderr, "usage: %s dir min_intv max_intv min_span split_len split_width\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    const uint32_t p[5] = { (uint32_t)strtoul( argv[2], 0, 0 ), (uint32_t)strtoul( argv[3], 0, 0 ), (uint32_t)strtoul( argv[4], 0, 0 ),
                            (uint32_t)strtoul( argv[5], 0, 0 ), (uint32_t)strtoul( argv[6], 0, 0 ) };
    try
    {
        const std::vector<uint8_t>  text    = load<uint8_t>( dir + "/text.u8" );
        std::vector<uint8_t>        reads   = load<uint8_t>( dir + "/reads.u8" );
        const std::vector<uint32_t> offsets = load<uint32_t>( dir + "/offsets.u32" );
        const std::vector<uint8_t>  rtext( text.rbegin(), text.rend() );
        device_vector<uint32_t> t2( pack2( text ) ), r2( pack2( rtext ) );
        fm_index f( t2.data(), (uint32_t)text.size(), 0, 0u, 0, 4u ), r( r2.data(), (uint32_t)text.size(), 0, 0u, 0, 4u );
        reads.resize( reads.size() + 16, 0 );
        device_vector<uint8_t>  d_reads( reads );
        device_vector<uint32_t> d_offs( offsets );
        const string_set set = string_set::concatenated( d_reads.data(), 8u, d_offs.data(), (uint32_t)offsets.size() - 1u );

        MEMFilter<amd_device_tag> filter;
        const uint64_t n_mems = filter.rank( f, r, set, p[0], p[1], p[2], p[3], p[4] );
        device_vector<nvbio_mem_hit> hits( n_mems );
        filter.locate( 0, n_mems, hits.data() );
        check_hip( hipDeviceSynchronize(), "locate" );

        std::vector<uint32_t> ranges( 4u * filter.n_ranges() ), first( set.size() + 1u );
        std::vector<uint64_t> slots( filter.n_ranges() );
        if (filter.n_ranges())
        {
            check_hip( hipMemcpy( ranges.data(), filter.mem_ranges(), ranges.size() * 4u, hipMemcpyDeviceToHost ), "ranges" );
            check_hip( hipMemcpy( slots.data(), filter.slots(), slots.size() * 8u, hipMemcpyDeviceToHost ), "slots" );
        }
        check_hip( hipMemcpy( first.data(), filter.first_ranges(), first.size() * 4u, hipMemcpyDeviceToHost ), "first" );
        const std::vector<nvbio_mem_hit> h = hits.to_host();
        std::vector<uint32_t> hw( 4u * h.size() );
        if (!h.empty()) memcpy( hw.data(), h.data(), hw.size() * 4u );
        save( dir + "/ranges.u32", ranges ); save( dir + "/first.u32", first ); save( dir + "/slots.u64", slots ); save( dir + "/hits.u32", hw );
        // first_hit agrees with the slots
        for (uint32_t s = 0; s <= set.size(); s += (set.size() / 7u) + 1u)
        {
            const uint64_t want = s >= set.size() ? n_mems : (first[s] ? slots[first[s] - 1u] : 0u);
            if (filter.first_hit( s ) != want) { fprintf( stderr, "first_hit(%u) mismatch\n", s ); return 1; }
        }
        printf( "mem filter ok: %u ranges, %llu mems\n", filter.n_ranges(), (unsigned long long)n_mems );
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
    return 0;
}
