// fasta.hpp -- reference FASTA input over the C ABI (nvbio_fasta_scan / nvbio_fasta_encode / nvbio_fasta_finish): what nvBWT's front half does
// on the host one byte at a time (FASTA_inc_reader::read, nvbio/fasta/fasta_inl.h:64-122, feeding the Writer of nvBWT/nvBWT.cu:102-195),
// done on the device -- the host is left with fread into pinned memory and one copy per chunk.
//
//   nvbio_amd::FastaFile ref( "genome.fa" );                      // or ref.read( "more.fa" ) for further files through the same state
//   ref.finish();
//   const nvbio_amd::FastaParser& r = ref.reference();            // r.text2(), r.length(), r.seq_offset(), r.names(), r.name_index(), the holes
//   nvbio_sam_refs refs = r.sam_refs();
//
// The grammar and its departures from the reference are listed in nvbio_amd.h ("FASTA input").  Header-only; needs nvbio_amd.hpp.
#pragma once

#include <nvbio_amd/nvbio_amd.hpp>
#include <cstdio>
#include <string>

namespace nvbio_amd {

// chunks of text on the device, cut anywhere, appended to one reference on the device
class FastaParser
{
public:
    explicit FastaParser(int device = 0, uint32_t seed = 11u, hipStream_t stream = 0)
        : m_device( device ), m_state(), m_last(), m_state_dev( 1u ), m_summary_dev( 1u ), m_status_dev( 1u ), m_seqs( 0 ), m_holes( 0 ), m_names_used( 0 )
    {
        check( nvbio_fasta_state_init( m_device, m_state_dev.data(), seed, stream ) );
        check_hip( hipMemsetAsync( m_status_dev.data(), 0, sizeof(uint32_t), stream ), "hipMemsetAsync" );
    }

    // room for a text of this many symbols (symbols <= bytes of FASTA); what is there is kept
    void reserve_symbols(uint64_t symbols) { const size_t words = (size_t)((symbols + 15u) / 16u) + 4u; if (m_text2.size() < words) m_text2.resize( words ); }

    // the next chunk: text_dev[0, text_bytes) (device memory, 16-byte aligned, below 4 GiB).  Synchronises `stream` once, for the summary,
    // from which the arrays grow.  Returns the chunk's summary; END_BYTE in its status says that the input has ended.
    const nvbio_fasta_summary& push(const uint8_t* text_dev, uint64_t text_bytes, hipStream_t stream = 0)
    {
        uint64_t temp_bytes = 0;
        check( nvbio_fasta_temp_bytes( text_bytes, &temp_bytes ) );
        if (m_temp.size() < temp_bytes) m_temp.resize( temp_bytes );
        check( nvbio_fasta_scan( m_device, text_dev, text_bytes, m_state_dev.data(), m_summary_dev.data(), m_temp.data(), m_temp.size(), stream ) );
        check_hip( hipMemcpyAsync( &m_last, m_summary_dev.data(), sizeof(m_last), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        if (m_last.status & NVBIO_FASTA_STATUS_OVERFLOW_32) throw error( NVBIO_ERR_UNSUPPORTED, "FastaParser: the symbols or name bytes reach 2^32" );
        m_symbols += m_last.n_symbols;
        reserve_symbols( m_symbols );
        grow( m_seq_offset, m_seqs + m_last.n_seqs + 1u ); grow( m_name_index, m_seqs + m_last.n_seqs + 1u );
        grow( m_names, m_names_used + m_last.n_name_bytes );
        grow( m_hole_offset, m_holes + m_last.n_holes ); grow( m_hole_rank, m_holes + m_last.n_holes ); grow( m_hole_amb, m_holes + m_last.n_holes );
        check( nvbio_fasta_encode( m_device, text_dev, text_bytes, m_temp.data(), m_temp.size(), m_state_dev.data(), m_text2.data(), m_text2.size(),
                                   m_seq_offset.data(), m_name_index.data(), (uint32_t)m_seq_offset.size() - 1u, m_names.data(), m_names.size(),
                                   m_hole_offset.data(), m_hole_rank.data(), m_hole_amb.data(), (uint32_t)m_hole_offset.size(), m_status_dev.data(), stream ) );
        m_seqs += m_last.n_seqs; m_holes += m_last.n_holes; m_names_used += m_last.n_name_bytes;
        return m_last;
    }

    // closes the tables behind the last chunk and reads the state back.  Synchronises `stream`.
    const nvbio_fasta_state& finish(hipStream_t stream = 0)
    {
        grow( m_hole_len, m_holes ); grow( m_seq_n_ambs, m_seqs );
        check( nvbio_fasta_finish( m_device, m_state_dev.data(), m_seq_offset.data(), m_name_index.data(), (uint32_t)m_seq_offset.size() - 1u, m_hole_offset.data(),
                                   m_hole_rank.data(), (uint32_t)m_hole_offset.size(), m_hole_len.data(), m_seq_n_ambs.data(), stream ) );
        uint32_t status = 0;
        check_hip( hipMemcpyAsync( &m_state, m_state_dev.data(), sizeof(m_state), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipMemcpyAsync( &status, m_status_dev.data(), sizeof(status), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        if (status & NVBIO_FASTA_STATUS_CAPACITY) throw error( NVBIO_ERR_INVALID, "nvbio_fasta_encode: an item did not fit arrays sized from the summaries" );
        return m_state;
    }

    const nvbio_fasta_state&   state() const        { return m_state; }            // after finish()
    const nvbio_fasta_summary& last_summary() const { return m_last; }
    uint32_t        length() const      { return m_state.n_symbols; }
    uint32_t        n_seqs() const      { return m_state.n_seqs; }
    uint32_t        n_holes() const     { return m_state.n_holes; }
    const uint32_t* text2() const       { return m_text2.data(); }                 // ceil( length / 16 ) words
    const uint32_t* seq_offset() const  { return m_seq_offset.data(); }            // n_seqs + 1
    const uint32_t* name_index() const  { return m_name_index.data(); }            // n_seqs + 1
    const uint8_t*  names() const       { return m_names.data(); }
    const uint32_t* seq_n_ambs() const  { return m_seq_n_ambs.data(); }            // n_seqs
    const uint32_t* hole_offset() const { return m_hole_offset.data(); }           // n_holes each
    const uint32_t* hole_len() const    { return m_hole_len.data(); }
    const uint8_t*  hole_amb() const    { return m_hole_amb.data(); }
    nvbio_sam_refs  sam_refs() const    { return nvbio_sam_refs{ m_state.n_seqs, m_state.max_name_len, m_seq_offset.data(), m_names.data(), m_name_index.data() }; }
    int             device() const      { return m_device; }

private:
    template <typename T> static void grow(device_vector<T>& v, size_t need) { if (v.size() < need || v.size() == 0) v.resize( need > 2u * v.size() ? (need ? need : 1u) : 2u * v.size() ); }

    int                                m_device;
    nvbio_fasta_state                  m_state;
    nvbio_fasta_summary                m_last;
    device_vector<nvbio_fasta_state>   m_state_dev;
    device_vector<nvbio_fasta_summary> m_summary_dev;
    device_vector<uint32_t>            m_status_dev, m_text2, m_seq_offset, m_name_index, m_hole_offset, m_hole_rank, m_hole_len, m_seq_n_ambs;
    device_vector<uint8_t>             m_temp, m_names, m_hole_amb;
    uint64_t                           m_symbols = 0;
    size_t                             m_seqs, m_holes, m_names_used;
};

// FASTA files read in chunks through one FastaParser: fread into pinned memory, one copy to the device per chunk
class FastaFile
{
public:
    explicit FastaFile(const char* path = nullptr, size_t chunk_bytes = 64u << 20, int device = 0, uint32_t seed = 11u)
        : m_parser( device, seed ), m_chunk( chunk_bytes ? chunk_bytes : 1u ), m_host( nullptr ), m_ended( false )
    {
        if (path) read( path );
    }
    FastaFile(const FastaFile&) = delete;
    FastaFile& operator=(const FastaFile&) = delete;
    ~FastaFile() { if (m_host) (void)hipHostFree( m_host ); }

    // the whole file at `path`, appended to what was read before
    void read(const char* path, hipStream_t stream = 0)
    {
        FILE* fp = fopen( path, "rb" );
        if (!fp) throw error( NVBIO_ERR_INVALID, std::string( "FastaFile: cannot open " ) + path );
        try
        {
            if (!m_host) check_hip( hipHostMalloc( (void**)&m_host, m_chunk, hipHostMallocDefault ), "hipHostMalloc" );
            if (m_text.size() < m_chunk) m_text.resize( m_chunk );
            for (size_t got; !m_ended && (got = fread( m_host, 1, m_chunk, fp )) > 0; )
            {
                check_hip( hipMemcpyAsync( m_text.data(), m_host, got, hipMemcpyHostToDevice, stream ), "hipMemcpyAsync H2D" );
                m_ended = (m_parser.push( m_text.data(), got, stream ).status & NVBIO_FASTA_STATUS_END_BYTE) != 0u;     // synchronises: the pinned buffer is free again
            }
        }
        catch (...) { fclose( fp ); throw; }
        fclose( fp );
    }

    // behind the last file.  Throws when the input ended inside a header line.
    const FastaParser& finish(hipStream_t stream = 0)
    {
        m_parser.finish( stream );
        if (m_parser.last_summary().status & NVBIO_FASTA_STATUS_INCOMPLETE) throw error( NVBIO_ERR_INVALID, "FastaFile: the input ends inside a header line" );
        return m_parser;
    }
    const FastaParser& reference() const { return m_parser; }

private:
    FastaParser            m_parser;
    size_t                 m_chunk;
    uint8_t*               m_host;                       // pinned
    bool                   m_ended;
    device_vector<uint8_t> m_text;
};

} // namespace nvbio_amd
