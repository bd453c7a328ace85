// fastq.hpp -- FASTQ input over the C ABI (nvbio_fastq_scan / nvbio_fastq_encode): what io::open_sequence_file + SequenceDataFile::next
// (nvbio/io/sequence/sequence.h:629-660, sequence_fastq.cpp:39-203, sequence_encoder.cpp:304-368) do on the host, one byte and one read
// at a time, done on the device -- the host is left with fread into pinned memory and one copy per chunk.
//
//   nvbio_amd::FastqFile file( "reads.fq" );                       // Phred33, NO_OP; nvBowtie loads with NVBIO_FASTQ_REVERSE_OP
//   while (file.next_batch( 1u << 20 ))
//   {
//       const nvbio_amd::FastqParser& b = file.batch();            // b.n_records() reads: b.reads4(), b.read_index(), b.quals(), b.names(), b.name_index()
//       ...
//   }
//
// The grammar and its departures from the reference are listed in nvbio_amd.h ("FASTQ input").  Header-only; needs nvbio_amd.hpp.
#pragma once

#include <nvbio_amd/nvbio_amd.hpp>
#include <cstdio>
#include <cstring>
#include <string>

namespace nvbio_amd {

// one chunk of text on the device -> one batch on the device, in buffers that are kept from chunk to chunk
class FastqParser
{
public:
    explicit FastqParser(int device = 0, uint32_t quality_encoding = NVBIO_FASTQ_PHRED33, uint32_t strand_op = NVBIO_FASTQ_NO_OP,
                         uint32_t truncate_len = 0xFFFFFFFFu)
        : m_device( device ), m_params{ quality_encoding, strand_op, truncate_len, 0xFFFFFFFFu }, m_summary() {}

    // the records of text_dev[0, text_bytes) (device memory, 16-byte aligned, below 4 GiB), at most max_records of them.  Synchronises
    // `stream` twice: for the summary, from which the arrays are sized, and for the status word.  Errors in the TEXT do not throw: see
    // summary().status and summary().consumed_bytes.
    const nvbio_fastq_summary& parse(const uint8_t* text_dev, uint64_t text_bytes, uint32_t max_records = 0xFFFFFFFFu, hipStream_t stream = 0)
    {
        m_params.max_records = max_records;
        uint64_t temp_bytes = 0;
        check( nvbio_fastq_temp_bytes( text_bytes, max_records, &temp_bytes ) );
        if (m_temp.size() < temp_bytes) m_temp.resize( temp_bytes );
        if (m_summary_dev.size() < 1u) m_summary_dev.resize( 1u );
        check( nvbio_fastq_scan( m_device, text_dev, text_bytes, &m_params, m_summary_dev.data(), m_temp.data(), m_temp.size(), stream ) );
        check_hip( hipMemcpyAsync( &m_summary, m_summary_dev.data(), sizeof(m_summary), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        const size_t words = ((size_t)m_summary.n_symbols + 7u) / 8u, n = m_summary.n_records;
        if (m_reads4.size() < words) m_reads4.resize( words );
        if (m_quals.size() < 8u * words) m_quals.resize( 8u * words );
        if (m_names.size() < m_summary.n_name_bytes) m_names.resize( m_summary.n_name_bytes );
        if (m_read_index.size() < n + 1u) { m_read_index.resize( n + 1u ); m_name_index.resize( n + 1u ); }
        check( nvbio_fastq_encode( m_device, text_dev, text_bytes, &m_params, m_temp.data(), m_temp.size(), m_reads4.data(), words, m_read_index.data(),
                                   m_quals.data(), m_names.data(), m_summary.n_name_bytes, m_name_index.data(), &m_summary_dev.data()->status, stream ) );
        check_hip( hipMemcpyAsync( &m_summary.status, &m_summary_dev.data()->status, sizeof(uint32_t), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        if (m_summary.status & NVBIO_FASTQ_STATUS_CAPACITY) throw error( NVBIO_ERR_INVALID, "nvbio_fastq_encode: a record did not fit arrays sized from the summary" );
        return m_summary;
    }

    const nvbio_fastq_summary& summary() const { return m_summary; }
    uint32_t        n_records() const  { return m_summary.n_records; }
    const uint32_t* reads4() const     { return m_reads4.data(); }        // ceil( n_symbols / 8 ) words
    const uint32_t* read_index() const { return m_read_index.data(); }    // n_records + 1
    const uint8_t*  quals() const      { return m_quals.data(); }         // n_symbols
    const uint8_t*  names() const      { return m_names.data(); }         // n_name_bytes
    const uint32_t* name_index() const { return m_name_index.data(); }    // n_records + 1
    int             device() const     { return m_device; }

private:
    int                                m_device;
    nvbio_fastq_params                 m_params;
    nvbio_fastq_summary                m_summary;
    device_vector<nvbio_fastq_summary> m_summary_dev;
    device_vector<uint8_t>             m_temp, m_quals, m_names;
    device_vector<uint32_t>            m_reads4, m_read_index, m_name_index;
};

// a FASTQ file read in chunks: fread into pinned memory, one copy to the device, parse, and the bytes the parse did not consume (the
// record a chunk cuts, or what a max_records cap left) carried in front of the next chunk
class FastqFile
{
public:
    explicit FastqFile(const char* path, size_t chunk_bytes = 64u << 20, int device = 0, uint32_t quality_encoding = NVBIO_FASTQ_PHRED33,
                       uint32_t strand_op = NVBIO_FASTQ_NO_OP, uint32_t truncate_len = 0xFFFFFFFFu)
        : m_parser( device, quality_encoding, strand_op, truncate_len ), m_fp( fopen( path, "rb" ) ), m_chunk( chunk_bytes ? chunk_bytes : 1u ),
          m_host( nullptr ), m_cap( 0 ), m_fill( 0 ), m_eof( false ), m_fresh( false )
    {
        if (!m_fp) throw error( NVBIO_ERR_INVALID, std::string( "FastqFile: cannot open " ) + path );
    }
    FastqFile(const FastqFile&) = delete;
    FastqFile& operator=(const FastqFile&) = delete;
    ~FastqFile() { if (m_fp) fclose( m_fp ); if (m_host) (void)hipHostFree( m_host ); }

    // the next batch, of at most max_records (> 0) reads, into batch(); false at the end of the file.  A chunk that holds no whole record
    // is extended by the next.  Throws on a marker error, and at the end of the file on an unfinished record: the reference's "incomplete read".
    bool next_batch(uint32_t max_records = 0xFFFFFFFFu, hipStream_t stream = 0)
    {
        for (;;)
        {
            if (!m_eof && !m_fresh)                                                // m_fresh: a cap left whole records in the buffer; parse them first
            {
                reserve( m_fill + m_chunk );
                const size_t got = fread( m_host + m_fill, 1, m_chunk, m_fp );
                m_fill += got;
                if (got < m_chunk) m_eof = true;
            }
            if (m_fill == 0) return false;
            if (m_text.size() < m_fill) m_text.resize( m_fill );
            check_hip( hipMemcpyAsync( m_text.data(), m_host, m_fill, hipMemcpyHostToDevice, stream ), "hipMemcpyAsync H2D" );
            const nvbio_fastq_summary& s = m_parser.parse( m_text.data(), m_fill, max_records, stream );     // synchronises: the pinned buffer is free again
            if (s.status & NVBIO_FASTQ_STATUS_MARKER)
                throw error( NVBIO_ERR_INVALID, "FastqFile: parse error: byte " + std::to_string( s.error_char ) + " where a record must begin with '@'" );
            memmove( m_host, m_host + s.consumed_bytes, m_fill - s.consumed_bytes );
            m_fill -= s.consumed_bytes;
            m_fresh = s.n_records == max_records && m_fill > 0;
            if (s.n_records) return true;
            if (m_eof)
            {
                if (s.status & NVBIO_FASTQ_STATUS_INCOMPLETE) throw error( NVBIO_ERR_INVALID, "FastqFile: incomplete read at the end of the file" );
                return false;
            }
        }
    }
    const FastqParser& batch() const { return m_parser; }

private:
    void reserve(size_t bytes)
    {
        if (bytes <= m_cap) return;
        uint8_t* p = nullptr;
        check_hip( hipHostMalloc( (void**)&p, bytes, hipHostMallocDefault ), "hipHostMalloc" );
        if (m_fill) memcpy( p, m_host, m_fill );
        if (m_host) (void)hipHostFree( m_host );
        m_host = p; m_cap = bytes;
    }
    FastqParser            m_parser;
    FILE*                  m_fp;
    size_t                 m_chunk;
    uint8_t*               m_host;                       // pinned: [0, m_fill) = the carried tail and what was read behind it
    size_t                 m_cap, m_fill;
    bool                   m_eof, m_fresh;
    device_vector<uint8_t> m_text;
};

} // namespace nvbio_amd
