// The C++ host loop of nvBowtie's all-mapping mode (nvbio_amd/all_mapping.hpp) over files written by tests/test_gpu_all_mapping_cpp.py:
//   test_all_mapping <dir> <n_reads> <read_len> <aln_type> <max_dist> <hits_per_batch> <unique> <per_seed_passes> <capacity>
// reads <dir>/text.u8 (symbols 0..3) and <dir>/stored.u8 (the reads as nvBowtie stores them -- reversed --, one symbol per byte, N = 4),
// builds the index on the GPU, runs the loop with CIGARs and the per-chunk callback, and writes records.u32 (n x 4: read_id, rc, loc, score),
// details.u32 (n x 5: source.x, source.y, sink.x, sink.y, ed), cigars.u16 (n x 64), cigar_lens.u32, the same records as the callback saw
// them chunk by chunk (cb_records.u32, cb_first.u64) and stats.u64 (n_hits, n_scored, n_alignments, chunks).
#include <nvbio_amd/nvbio_amd.hpp>
#include <nvbio_amd/all_mapping.hpp>
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
    if (argc != 10) { fprintf( stderr, "usage: %s dir n_reads read_len aln_type max_dist hits_per_batch unique per_seed_passes capacity\n", argv[0] ); return 2; }
    const std::string dir = argv[1];
    uint32_t a[8];
    for (int i = 0; i < 8; ++i) a[i] = (uint32_t)strtoul( argv[2 + i], 0, 0 );
    const uint32_t R = a[0], M = a[1], cap = a[7], stride = 64;
    try
    {
        const std::vector<uint8_t> text = load<uint8_t>( dir + "/text.u8" ), stored = load<uint8_t>( dir + "/stored.u8" );
        if (stored.size() != (size_t)R * M) { fprintf( stderr, "stored.u8 does not hold n_reads x read_len symbols\n" ); return 1; }
        device_vector<uint32_t> t2( pack<2>( text ) ), r4( pack<4>( stored ) );
        fm_index f( t2.data(), (uint32_t)text.size(), 0, 8u, 0, 4u );

        AllMappingParams prm;
        prm.aln_type = (nvbio_alignment_type)a[2]; prm.max_dist = a[3]; prm.hits_per_batch = a[4]; prm.unique = a[5]; prm.per_seed_passes = a[6];
        prm.want_cigars = 1;
        device_vector<uint32_t> o_read( cap ), o_loc( cap ), o_wb( cap ), o_ed( cap ), o_lens( cap );
        device_vector<uint8_t> o_rc( cap );
        device_vector<int32_t> o_score( cap );
        device_vector<nvbio_uint2> o_src( cap ), o_sink( cap );
        device_vector<uint16_t> o_cig( (size_t)cap * stride );
        AllMappingOutput out;
        out.capacity = cap; out.read_id = o_read.data(); out.rc = o_rc.data(); out.loc = o_loc.data(); out.score = o_score.data(); out.win_begin = o_wb.data();
        out.source = o_src.data(); out.sink = o_sink.data(); out.ed = o_ed.data(); out.cigars = o_cig.data(); out.cigar_stride = stride; out.cigar_lens = o_lens.data();

        std::vector<uint32_t> cb_records; std::vector<uint64_t> cb_first;
        const nvbio_sw_scheme ed_scheme = { 0, -1, -1, -1 };
        const AllMappingStats st = all_mapping( 0, f.handle(), t2.data(), (uint32_t)text.size(), r4.data(), R, M, ed_scheme, -(int32_t)prm.max_dist, prm, out, 0,
            [&](const AllMappingChunk& c)
            {
                check_hip( hipStreamSynchronize( 0 ), "chunk" );
                const std::vector<uint32_t> rid = fetch( c.read_id, c.n ), loc = fetch( c.loc, c.n ), ed = fetch( c.ed, c.n );
                const std::vector<uint8_t>  rc = fetch( c.rc, c.n );
                const std::vector<int32_t>  sc = fetch( c.score, c.n );
                cb_first.push_back( c.first ); cb_first.push_back( c.n );
                for (uint32_t i = 0; i < c.n; ++i) { cb_records.push_back( rid[i] ); cb_records.push_back( rc[i] ); cb_records.push_back( loc[i] ); cb_records.push_back( (uint32_t)sc[i] ); cb_records.push_back( ed[i] ); }
            } );

        const size_t n = st.n_alignments < cap ? (size_t)st.n_alignments : cap;
        const std::vector<uint32_t> rid = fetch( o_read.data(), n ), loc = fetch( o_loc.data(), n ), ed = fetch( o_ed.data(), n ), lens = fetch( o_lens.data(), n );
        const std::vector<uint8_t>  rc = fetch( o_rc.data(), n );
        const std::vector<int32_t>  sc = fetch( o_score.data(), n );
        const std::vector<nvbio_uint2> src = fetch( o_src.data(), n ), snk = fetch( o_sink.data(), n );
        std::vector<uint32_t> records, details;
        for (size_t i = 0; i < n; ++i)
        {
            records.push_back( rid[i] ); records.push_back( rc[i] ); records.push_back( loc[i] ); records.push_back( (uint32_t)sc[i] );
            details.push_back( src[i].x ); details.push_back( src[i].y ); details.push_back( snk[i].x ); details.push_back( snk[i].y ); details.push_back( ed[i] );
        }
        save( dir + "/records.u32", records ); save( dir + "/details.u32", details ); save( dir + "/cigars.u16", fetch( o_cig.data(), n * stride ) );
        save( dir + "/cigar_lens.u32", lens ); save( dir + "/cb_records.u32", cb_records ); save( dir + "/cb_first.u64", cb_first );
        save( dir + "/stats.u64", std::vector<uint64_t>{ st.n_hits, st.n_scored, st.n_alignments, st.chunks } );
        printf( "all mapping ok: %llu hits, %llu scored, %llu alignments, %u chunks\n", (unsigned long long)st.n_hits, (unsigned long long)st.n_scored,
                (unsigned long long)st.n_alignments, st.chunks );
    }
    catch (const std::exception& e)
    {
        fprintf( stderr, "%s\n", e.what() );
        return 1;
    }
    return 0;
}
