// sam.hpp -- SAM output over the C ABI (nvbio_sam_record_offsets / nvbio_sam_format): what io::SamOutput
// (nvbio/io/output/output_sam.cpp:155-178 the header, :182-544 the records) does on the host, one fwrite per field, done on the
// device in three steps -- record offsets, one read of the total, the text -- so that the host is left with one fwrite of one buffer.
//
//   nvbio_amd::SamFormatter fmt;
//   fmt.format( refs, records );                        // refs / records: nvbio_sam_refs / nvbio_sam_records over device arrays
//   fputs( nvbio_amd::sam_header( names, lengths ).c_str(), fp );
//   fmt.write( fp );                                    // fmt.bytes() bytes; fmt.n_skipped() records took none
//
// Header-only; needs nvbio_amd.hpp (device_vector, check).
#pragma once

#include <nvbio_amd/nvbio_amd.hpp>
#include <cstdio>
#include <string>
#include <vector>

namespace nvbio_amd {

// SamOutput::output_header (output_sam.cpp:155-178): @HD VN:1.3, @PG with the reference's ID / PN / VN unless told otherwise, one @SQ per sequence
inline std::string sam_header(const std::vector<std::string>& names, const std::vector<uint32_t>& lengths, const std::string& pg_id = "nvBowtie",
                              const std::string& pg_name = "nvBowtie", const std::string& pg_version = "0.5.1")
{
    std::string h = "@HD\tVN:1.3\n@PG\tID:" + pg_id + "\tPN:" + pg_name + "\tVN:" + pg_version + "\n";
    for (size_t i = 0; i < names.size() && i < lengths.size(); ++i) h += "@SQ\tSN:" + names[i] + "\tLN:" + std::to_string( lengths[i] ) + "\n";
    return h;
}

// offsets -> allocate -> format, with buffers that are kept from batch to batch
class SamFormatter
{
public:
    explicit SamFormatter(int device = 0) : m_device( device ), m_n( 0 ), m_bytes( 0 ), m_skipped( 0 ) {}

    // the text of `records` on the device: text() holds bytes() bytes, record i at [offsets()[i], offsets()[i + 1]).  Synchronises `stream` twice:
    // for the total, and for the count of skipped records and the status word (a set bit throws).
    void format(const nvbio_sam_refs& refs, const nvbio_sam_records& records, hipStream_t stream = 0)
    {
        m_n = records.n;
        uint64_t temp_bytes = 0;
        check( nvbio_sam_format_temp_bytes( m_n, &temp_bytes ) );
        if (m_temp.size() < temp_bytes) m_temp.resize( temp_bytes );
        if (m_offsets.size() < (size_t)m_n + 1u) m_offsets.resize( (size_t)m_n + 1u );
        if (m_words.size() < 2u) m_words.resize( 2u );
        check( nvbio_sam_record_offsets( m_device, &refs, &records, 0u, m_offsets.data(), m_temp.data(), temp_bytes, stream ) );
        check_hip( hipMemcpyAsync( &m_bytes, m_offsets.data() + m_n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        if (m_text.size() < m_bytes) m_text.resize( (size_t)m_bytes );
        check_hip( hipMemsetAsync( m_words.data(), 0, 2u * sizeof(uint32_t), stream ), "hipMemsetAsync" );
        check( nvbio_sam_format( m_device, &refs, &records, 0u, m_offsets.data(), m_text.data(), m_bytes, m_words.data(), m_words.data() + 1, stream ) );
        uint32_t words[2] = { 0u, 0u };
        check_hip( hipMemcpyAsync( words, m_words.data(), sizeof(words), hipMemcpyDeviceToHost, stream ), "hipMemcpyAsync D2H" );
        check_hip( hipStreamSynchronize( stream ), "hipStreamSynchronize" );
        m_skipped = words[0];
        if (words[1]) throw std::runtime_error( "nvbio_sam_format: status " + std::to_string( words[1] ) + " (NVBIO_SAM_STATUS_*)" );
    }

    const uint8_t*  text() const      { return m_text.data(); }
    const uint64_t* offsets() const   { return m_offsets.data(); }
    uint64_t        bytes() const     { return m_bytes; }
    uint32_t        n_skipped() const { return m_skipped; }

    // the text to the host (one copy) and to `fp` (one fwrite); returns the bytes written
    size_t write(FILE* fp)
    {
        m_host.resize( (size_t)m_bytes );
        if (m_bytes) check_hip( hipMemcpy( m_host.data(), m_text.data(), (size_t)m_bytes, hipMemcpyDeviceToHost ), "hipMemcpy D2H" );
        return m_bytes ? fwrite( m_host.data(), 1, (size_t)m_bytes, fp ) : 0u;
    }

private:
    int                     m_device;
    uint32_t                m_n;
    uint64_t                m_bytes;
    uint32_t                m_skipped;
    device_vector<uint64_t> m_offsets;
    device_vector<uint8_t>  m_temp, m_text;
    device_vector<uint32_t> m_words;                    // n_skipped | status
    std::vector<uint8_t>    m_host;
};

} // namespace nvbio_amd
