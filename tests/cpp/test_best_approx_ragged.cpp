// The C++ host loop of nvBowtie's best-approx mode over reads of different lengths (nvbio_amd/best_approx.hpp: best_approx_ragged) over files written by
// tests/test_gpu_best_approx_ragged_cpp.py:
//   test_best_approx_ragged <dir> <n_reads> <aln_type> <batch_size> <multi_hit> <tight>
// reads <dir>/text.u8 (symbols 0..3), <dir>/stored.u8 (the reads as nvBowtie stores them -- reversed --, back to back, one symbol per byte, N = 4),
// <dir>/offsets.u32 (n_reads + 1 symbol offsets) and <dir>/min_scores.i32 (every read's worst score), builds the index on the GPU, runs the loop with
// nvBowtie's end-to-end scheme and writes best.i32 (n x 4: a1 score, a1 locus, a2 score, a2 locus), best_rc.u8 and stats.u64 (n_extensions, passes,
// multi_passes, seeding_passes).  With <tight> the effort parameters of the parity tests' "tight" set.  A batch the loop refuses (a read of 1024
// symbols or more) prints "refused: <reason>", writes the untouched result arrays and returns 3.
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
        const std::vector<uint8_t> text = load<uint8_t>( dir + "/text.u8" ), stored = load<uint8_t>( dir + "/stored.u8" );
        const std::vector<uint32_t> offsets = load<uint32_t>( dir + "/offsets.u32" );
        const std::vector<int32_t> min_scores = load<int32_t>( dir + "/min_scores.i32" );
        if (offsets.size() != (size_t)R + 1 || min_scores.size() != R || stored.size() != offsets[R]) { fprintf( stderr, "the input files do not fit n_reads\n" ); return 1; }
        device_vector<uint32_t> t2( pack<2>( text ) ), r4( pack<4>( stored ) );
        fm_index f( t2.data(), (uint32_t)text.size(), 0, 8u, 0, 16u );

        BestApproxParams prm;
        prm.batch_size = a[2]; prm.multi_hit = a[3];
        if (a[4]) { prm.max_hits = 6; prm.rep_seeds = 8; prm.max_effort = 2; prm.min_ext = 3; prm.max_ext = 12; }
        const nvbio_gotoh_scheme scheme = { 0, 6, 6, -8, -3, -8, -3 };
        device_vector<int32_t> best( std::vector<int32_t>( 4u * (size_t)R, 0x5A5A5A5A ) );
        device_vector<uint8_t> best_rc( std::vector<uint8_t>( R, (uint8_t)0xA5 ) );
        int ret = 0;
        BestApproxStats st;
        try { st = best_approx_ragged( 0, f.handle(), t2.data(), (uint32_t)text.size(), r4.data(), nullptr, R, offsets.data(), (nvbio_alignment_type)a[1], scheme,
                                       min_scores.data(), prm, best.data(), best_rc.data(), 0 ); }
        catch (const std::invalid_argument& e) { printf( "refused: %s\n", e.what() ); ret = 3; }
        check_hip( hipDeviceSynchronize(), "sync" );
        save( dir + "/best.i32", fetch( best.data(), 4u * (size_t)R ) ); save( dir + "/best_rc.u8", fetch( best_rc.data(), R ) );
        save( dir + "/stats.u64", std::vector<uint64_t>{ st.n_extensions, st.passes, st.multi_passes, st.seeding_passes } );
        if (ret == 0) printf( "best approx ragged ok: %llu extensions, %u passes, %u multi, %u seeding\n", (unsigned long long)st.n_extensions, st.passes, st.multi_passes, st.seeding_passes );
        return ret;
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
}
