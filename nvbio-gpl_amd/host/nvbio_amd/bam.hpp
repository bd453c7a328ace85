// bam.hpp -- BAM output over the C ABI (nvbio_bam_record_offsets / nvbio_bam_format / nvbio_bgzf_frame): what io::BamOutput
// (nvbio/io/output/output_bam.cpp:601-650 the header, :227-544 the records, :588-599 the blocks, :657-659 the EOF marker) does on the
// host, one record and one block after another, done on the device -- record offsets, one read of the total, the records, the BGZF
// blocks around them (stored DEFLATE blocks: uncompressed BAM) -- so that the host is left with one fwrite of one buffer.
//
//   nvbio_amd::BamFormatter fmt;
//   fmt.write_header( fp, nvbio_amd::bam_header( names, lengths ) );   // a block sequence of its own, as the reference writes it
//   fmt.format( refs, records );                        // refs / records: nvbio_sam_refs / nvbio_sam_records over device arrays
//   fmt.write( fp );                                    // frames the records and writes them; fmt.n_skipped() records took no bytes
//   fmt.write_eof( fp );
//
// Header-only; needs nvbio_amd.hpp (device_vector, check).
#pragma once

#include <nvbio_amd/nvbio_amd.hpp>
#include <cstdio>
#include <string>
#include <vector>

namespace nvbio_amd {

// the reference's two header lines (output_bam.cpp:616-623), with no NUL behind them
inline std::string bam_default_text() { return "@HD\tVN:1.3\n@PG\tID:nvBowtie\tPN:nvBowtie\tVN:0.5.1\n"; }

// BamOutput::output_header (output_bam.cpp:601-650): BAM\1, l_text, text, n_ref, then l_name, name + NUL, l_ref per sequence; pass
// sam_header( names, lengths ) as `text` for @SQ lines too
inline std::vector<uint8_t> bam_header(const std::vector<std::string>& names, const std::vector<uint32_t>& lengths, const std::string& text = bam_default_text())
{
    std::vector<uint8_t> h = { 'B', 'A', 'M', 1 };
    auto u32 = [&](const uint32_t v) { for (int k = 0; k < 4; ++k) h.push_back( (uint8_t)(v >> (8 * k)) ); };
    u32( (uint32_t)text.size() );
    h.insert( h.end(), text.begin(), text.end() );
    const size_t n = names.size() < lengths.size() ? names.size() : lengths.size();
    u32( (uint32_t)n );
    for (size_t i = 0; i < n; ++i)
    {
        u32( (uint32_t)names[i].size() + 1u );
        h.insert( h.end(), names[i].begin(), names[i].end() );
        h.push_back( 0 );
        u32( lengths[i] );
    }
    return h;
}

// the BGZF end-of-file marker (output_bam.cpp:657-659): an empty block
inline std::vector<uint8_t> bgzf_eof()
{
    return { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
}

// offsets -> allocate -> format -> frame, with buffers that are kept from batch to batch
class BamFormatter
{
public:
    explicit BamFormatter(int device = 0) : m_device( device ), m_n( 0 ), m_bytes( 0 ), m_framed( 0 ), m_skipped( 0 ) {}

    // the records on the device: data() holds bytes() bytes, record i at [offsets()[i], offsets()[i + 1]).  flags: 0 or NVBIO_BAM_REG2BIN.
    // Synchronises `stream` twice: for the total, and for the count of skipped records and the status word (a set bit throws).
    void format(const nvbio_sam_refs& refs, const nvbio_sam_records& records, uint32_t flags = 0u, hipStream_t stream = 0)
    {
        m_n = records.n;
        m_framed = 0;
        uint64_t temp_bytes = 0;
        check( nvbio_bam_format_temp_bytes( m_n, &temp_bytes ) );
        if (m_temp.size() < temp_bytes) m_temp.resize( temp_bytes );
        if (m_offsets.size() < (size_t)m_n + 1u) m_offsets.resize( (size_t)m_n + 1u );
        if (m_words.size() < 2u) m_words.resize( 2u );
        check( nvbio_bam_record_offsets( m_device, &refs, &records, flags, m_offsets.data(), m_temp.data(), temp_bytes, stream ) );
        check_hip( hipMemcpyAsync( &m_bytes, m_offsets.data() + m_n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        if (m_data.size() < m_bytes) m_data.resize( (size_t)m_bytes );
        check_hip( hipMemsetAsync( m_words.data(), 0, 2u * sizeof(uint32_t), stream ), "hipMemsetAsync" );
        check( nvbio_bam_format( m_device, &refs, &records, flags, m_offsets.data(), m_data.data(), m_bytes, m_words.data(), m_words.data() + 1, stream ) );
        uint32_t words[2] = { 0u, 0u };
        check_hip( hipMemcpyAsync( words, m_words.data(), sizeof(words), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        m_skipped = words[0];
        if (words[1]) throw std::runtime_error( "nvbio_bam_format: status " + std::to_string( words[1] ) + " (NVBIO_BAM_STATUS_*)" );
    }

    const uint8_t*  data() const      { return m_data.data(); }
    const uint64_t* offsets() const   { return m_offsets.data(); }
    uint64_t        bytes() const     { return m_bytes; }
    uint32_t        n_skipped() const { return m_skipped; }

    // the records as BGZF blocks on the device: framed() holds the returned number of bytes (0 for no records).  No synchronisation.
    uint64_t frame(hipStream_t stream = 0)
    {
        check( nvbio_bgzf_framed_bytes( m_bytes, &m_framed ) );
        if (m_out.size() < m_framed) m_out.resize( (size_t)m_framed );
        check( nvbio_bgzf_frame( m_device, m_data.data(), m_bytes, m_out.data(), m_framed, stream ) );
        return m_framed;
    }
    const uint8_t* framed() const { return m_out.data(); }

    // frame(), the blocks to the host (one copy) and to `fp` (one fwrite); returns the bytes written
    size_t write(FILE* fp, hipStream_t stream = 0)
    {
        frame( stream );
        return write_framed( fp, stream );
    }

    // `header` (bam_header) as a block sequence of its own, framed by the same device call; returns the bytes written.  The records of a
    // format() before it are kept; their frame is not.
    size_t write_header(FILE* fp, const std::vector<uint8_t>& header, hipStream_t stream = 0)
    {
        m_header.assign( header.data(), header.size() );
        check( nvbio_bgzf_framed_bytes( header.size(), &m_framed ) );
        if (m_out.size() < m_framed) m_out.resize( (size_t)m_framed );
        check( nvbio_bgzf_frame( m_device, m_header.data(), header.size(), m_out.data(), m_framed, stream ) );
        return write_framed( fp, stream );
    }

    size_t write_eof(FILE* fp) const { const std::vector<uint8_t> e = bgzf_eof(); return fwrite( e.data(), 1, e.size(), fp ); }

private:
    size_t write_framed(FILE* fp, hipStream_t stream)
    {
        m_host.resize( (size_t)m_framed );
        if (m_framed) check_hip( hipMemcpyAsync( m_host.data(), m_out.data(), (size_t)m_framed, hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        return m_framed ? fwrite( m_host.data(), 1, (size_t)m_framed, fp ) : 0u;
    }

    int                     m_device;
    uint32_t                m_n;
    uint64_t                m_bytes, m_framed;
    uint32_t                m_skipped;
    device_vector<uint64_t> m_offsets;
    device_vector<uint8_t>  m_temp, m_data, m_out, m_header;
    device_vector<uint32_t> m_words;                    // n_skipped | status
    std::vector<uint8_t>    m_host;
};

} // namespace nvbio_amd
