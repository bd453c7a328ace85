// The C++ host loop of nvBowtie's PAIRED best-approx mode over mates of different lengths (nvbio_amd/best_approx.hpp: best_approx_paired_ragged) over
// files written by tests/test_gpu_best_approx_paired_ragged_cpp.py:
//   test_best_approx_paired_ragged <dir> <n_reads> <aln_type> <batch_size> <multi_hit> <tight>
// reads <dir>/text.u8 (symbols 0..3) and, for m = 1, 2, <dir>/stored<m>.u8 (mate m of every pair as nvBowtie stores it -- reversed --, back to back, one
// symbol per byte, N = 4), <dir>/offsets<m>.u32 (n_reads + 1 symbol offsets) and <dir>/min_scores<m>.i32 (every mate's worst score), builds the index
// on the GPU, runs the loop with nvBowtie's end-to-end scheme and writes best_a.i32 / best_o.i32 (n x 2 x 4: score, position, sink offset, flags) and
// stats.u64 (n_extensions, n_opposite, passes, multi_passes).  With <tight> the effort and fragment parameters of the parity tests' "tight" set.  A
// batch the loop refuses (a mate of 1024 symbols or more) prints "refused: <reason>", writes the untouched result arrays and returns 3.
#include <nvbio_amd/nvbio_amd.hpp>
#include <nvbio_amd/best_approx.hpp>
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
// big-endian packing (PackedStream<uint32,BITS,true>), with padding words
template <uint32_t BITS>
static std::vector<uint32_t> pack(const std::vector<uint8_t>& s)
{
    const uint32_t per = 32u / BITS;
    std::vector<uint32_t> w( (s.size() + per - 1) / per + 4, 0u );
    for (size_t i = 0; i < s.size(); ++i) w[i / per] |= (uint32_t)(s[i] & ((1u << BITS) - 1u)) << (32u - BITS - BITS * (uint32_t)(i % per));
    return w;
}
template <typename T>
static std::vector<T> fetch(const T* dev, size_t n)
{
    std::vector<T> h( n );
    if (n) nvbio_amd::check_hip( hipMemcpy( h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost ), "hipMemcpy D2H" );
    return h;
}

int main(int argc, char** argv)
{
    using namespace nvbio_amd;
    using namespace nvbio_amd_host;
    if (argc != 7) { fprintf( stderr, "usage: %s dir n_reads aln_type batch_size multi_hit tight\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    uint32_t a[5];
    for (int i = 0; i < 5; ++i) a[i] = (uint32_t)strtoul( argv[2 + i], 0, 0 );
    const uint32_t R = a[0];
    try
    {
        const std::vector<uint8_t> text = load<uint8_t>( dir + "/text.u8" );
        const std::vector<uint8_t> stored[2] = { load<uint8_t>( dir + "/stored1.u8" ), load<uint8_t>( dir + "/stored2.u8" ) };
        const std::vector<uint32_t> offsets[2] = { load<uint32_t>( dir + "/offsets1.u32" ), load<uint32_t>( dir + "/offsets2.u32" ) };
        const std::vector<int32_t> min_scores[2] = { load<int32_t>( dir + "/min_scores1.i32" ), load<int32_t>( dir + "/min_scores2.i32" ) };
        for (int m = 0; m < 2; ++m)
            if (offsets[m].size() != (size_t)R + 1 || min_scores[m].size() != R || stored[m].size() != offsets[m][R]) { fprintf( stderr, "the input files do not fit n_reads\n" ); return 1; }
        device_vector<uint32_t> t2( pack<2>( text ) ), r1( pack<4>( stored[0] ) ), r2( pack<4>( stored[1] ) );
        fm_index f( t2.data(), (uint32_t)text.size(), 0, 8u, 0, 16u );

        BestApproxParams prm;
        PairedParams pe;
        prm.batch_size = a[2]; prm.multi_hit = a[3];
        if (a[4]) { prm.max_hits = 6; prm.rep_seeds = 8; prm.max_effort = 2; prm.min_ext = 3; prm.max_ext = 12; pe.min_frag_len = 150; pe.overlap = 0; }
        const nvbio_gotoh_scheme scheme = { 0, 6, 6, -8, -3, -8, -3 };
        device_vector<int32_t> best_a( std::vector<int32_t>( 8u * (size_t)R, 0x5A5A5A5A ) ), best_o( std::vector<int32_t>( 8u * (size_t)R, 0x5A5A5A5A ) );
        const uint32_t* reads[2] = { r1.data(), r2.data() }; const uint8_t* quals[2] = { nullptr, nullptr };
        const uint32_t* offs[2] = { offsets[0].data(), offsets[1].data() }; const int32_t* worst[2] = { min_scores[0].data(), min_scores[1].data() };
        int ret = 0;
        PairedStats st;
        try { st = best_approx_paired_ragged( 0, f.handle(), t2.data(), (uint32_t)text.size(), reads, quals, R, offs, (nvbio_alignment_type)a[1], scheme, worst, prm, pe,
                                              best_a.data(), best_o.data(), 0 ); }
        catch (const std::invalid_argument& e) { printf( "refused: %s\n", e.what() ); ret = 3; }
        check_hip( hipDeviceSynchronize(), "sync" );
        save( dir + "/best_a.i32", fetch( best_a.data(), 8u * (size_t)R ) ); save( dir + "/best_o.i32", fetch( best_o.data(), 8u * (size_t)R ) );
        save( dir + "/stats.u64", std::vector<uint64_t>{ st.n_extensions, st.n_opposite, st.passes, st.multi_passes } );
        if (ret == 0) printf( "best approx paired ragged ok: %llu extensions, %llu opposite, %u passes, %u multi\n", (unsigned long long)st.n_extensions,
                              (unsigned long long)st.n_opposite, st.passes, st.multi_passes );
        return ret;
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
}
