// bam.h -- unaligned (or aligned) BAM as a source of query reads for `taxor search` (SAMv1 section 4.2 over BGZF, section 4.1).
// What long-read basecallers write by default; the reference's users turn it into FASTQ with `samtools fastq` first, and the
// selection rules here are that command's defaults: secondary and supplementary records (flag & 0x900) are left out, a record
// stored reverse-complemented (flag & 0x10) is the read's reverse complement, the id is read_name.
// The host only WALKS the records: block_size, the fixed fields, the name, and the position of the 4-bit SEQ field.  The SEQ bytes
// of a batch are copied back to back into one buffer that goes to the device as it is (k_pack_nibbles, bam_pack.hip, turns them into
// the 2-bit words every other route produces and restores reversed reads there); CIGAR, QUAL and the tags are stepped over by
// arithmetic.  The inflated stream comes from GzMembers (BGZF is multi-member gzip) or from one zlib stream.
// Errors are thrown as std::runtime_error and name the record's ordinal.
#pragma once

#include "fastx.h"

#include <cstdio>

namespace bam {

enum Kind { NOT_BAM = 0, BAM = 1 };

// the 28 bytes every BGZF file ends with (SAMv1 section 4.1.2): an empty block
inline const unsigned char *eof_block()
{
    static const unsigned char b[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return b;
}

// length of the gzip header at p if it carries the BGZF extra subfield 'B' 'C' (SLEN 2), else 0
inline size_t bgzf_header_len(const unsigned char *p, size_t n)
{
    if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const size_t xlen = p[10] | ((size_t)p[11] << 8);
    if (12 + xlen > n) return 0;
    bool bc = false;
    for (size_t i = 12; i + 4 <= 12 + xlen;) {
        const size_t slen = p[i + 2] | ((size_t)p[i + 3] << 8);
        if (p[i] == 'B' && p[i + 1] == 'C' && slen == 2) bc = true;
        i += 4 + slen;
    }
    if (!bc || (p[3] & ~4u)) return 0;      // (BGZF sets FEXTRA alone: no name, comment or header CRC to step over)
    return 12 + xlen;
}

// What kind of query file is this, by content: BAM when the first gzip member is a BGZF block and the inflated stream begins with
// "BAM\1".  CRAM and SAM text are refused by name (throws), so is a BGZF stream that says "BAM" with another version byte.
// Anything else -- FASTA, FASTQ, their .gz (bgzip's output included) and .bz2 -- is NOT_BAM and goes to the FASTX readers.
inline Kind sniff(const std::string &path)
{
    // only a regular file is looked at: opening a pipe here would take its first bytes away from the reader that follows (and
    // closing it ends its writer).  Pipes and standard input go to the sequential FASTX reader as they always did
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return NOT_BAM;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return NOT_BAM;
    std::vector<unsigned char> head(1u << 16);
    head.resize(fread(head.data(), 1, head.size(), f));
    fclose(f);
    const unsigned char *p = head.data();
    const size_t n = head.size();
    if (n >= 4 && memcmp(p, "CRAM", 4) == 0)
        throw std::runtime_error("query file " + path + " is CRAM: not supported, convert it first (samtools fastq, or samtools view -b for unaligned BAM)");
    if (n >= 7 && p[0] == '@' && p[3] == '\t' && p[6] == ':' &&
        (!memcmp(p + 1, "HD", 2) || !memcmp(p + 1, "SQ", 2) || !memcmp(p + 1, "RG", 2) || !memcmp(p + 1, "PG", 2)))
        throw std::runtime_error("query file " + path + " is SAM text: not supported, convert it first (samtools view -b, or samtools fastq)");
    const size_t h = bgzf_header_len(p, n);
    if (!h) return NOT_BAM;
    unsigned char out[4] = {0, 0, 0, 0};
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return NOT_BAM;
    zs.next_in = const_cast<unsigned char *>(p + h);
    zs.avail_in = (uInt)(n - h);
    zs.next_out = out;
    zs.avail_out = 4;
    const int rc = inflate(&zs, Z_SYNC_FLUSH);
    const size_t got = 4 - zs.avail_out;
    inflateEnd(&zs);
    if ((rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) || got < 4 || memcmp(out, "BAM", 3) != 0) return NOT_BAM;
    if (out[3] != 1) throw std::runtime_error("query file " + path + ": wrong magic (BAM with version byte " + std::to_string((int)out[3]) + ", expected BAM\\1)");
    return BAM;
}

// the BAM alphabet (SAMv1 section 4.2.3) and the read a record stands for: the letters of its nibbles, for flag 0x10 the reverse
// complement on the IUPAC codes (the complement of a code is its four bits reversed: A=1 <-> T=8, C=2 <-> G=4)
inline const char *alphabet() { return "=ACMGRSVTWYHKDBN"; }
inline unsigned complement_nibble(unsigned x) { return ((x & 1) << 3) | ((x & 2) << 1) | ((x & 4) >> 1) | ((x & 8) >> 3); }
template <class Out> inline void restore_read(const uint8_t *seq4, uint32_t len, bool reverse, Out &out)
{
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t j = reverse ? len - 1 - i : i;
        unsigned x = (seq4[j >> 1] >> ((j & 1) ? 0 : 4)) & 15u;
        if (reverse) x = complement_nibble(x);
        const char c = alphabet()[x];
        out.append(&c, 1);
    }
}

struct Reader {
    // --- the inflated byte stream
    fastx::GzMembers members;
    bool use_members = false;
    gzFile gz = nullptr;
    const uint8_t *mem = nullptr;       // memory source (tests): the inflated stream itself
    size_t mem_len = 0, mem_pos = 0;
    std::vector<uint8_t> buf;
    size_t pos = 0, len = 0;
    bool src_eof = false;
    // --- counters
    uint64_t ordinal = 0;               // records met so far, skipped ones included (1-based in messages)
    uint64_t n_skipped = 0;             // secondary / supplementary
    std::function<void(size_t)> grow;   // called before the SEQ buffer must grow to hold at least that many bytes (the caller
                                        // may have page-locked it)
    std::string name;

    Reader() = default;
    Reader(const Reader &) = delete;
    Reader &operator=(const Reader &) = delete;
    ~Reader() { if (gz) gzclose(gz); }

    // threads > 1 and not sequential: the blocks are inflated in parallel (gzmembers.h); otherwise, and where that reader declines
    // (fewer than four blocks), one zlib stream.  Reads the header.  Warns on stderr when the BGZF end-of-file block is missing.
    void open(const std::string &path, unsigned threads, bool sequential)
    {
        name = path;
        buf.resize(4u << 20);
        if (FILE *f = fopen(path.c_str(), "rb")) {
            unsigned char tail[28];
            const bool has_eof = fseek(f, -28, SEEK_END) == 0 && fread(tail, 1, 28, f) == 28 && memcmp(tail, eof_block(), 28) == 0;
            fclose(f);
            if (!has_eof) fprintf(stderr, "[TAXOR SEARCH WARNING] %s: the BGZF end-of-file block is missing; the file may be truncated\n", path.c_str());
        }
        use_members = !sequential && members.open(path, std::max(1u, threads));
        if (!use_members) {
            gz = gzopen(path.c_str(), "rb");
            if (!gz) throw std::runtime_error("cannot open query file " + path);
            gzbuffer(gz, 1 << 20);
        }
        read_header();
    }
    void open_mem(const uint8_t *p, size_t n)
    {
        name = "(memory)";
        mem = p;
        mem_len = n;
        mem_pos = 0;
        buf.resize(1u << 16);
        read_header();
    }

    size_t source_read(uint8_t *dst, size_t n)
    {
        if (mem) {
            const size_t take = std::min(n, mem_len - mem_pos);
            if (take) memcpy(dst, mem + mem_pos, take);
            mem_pos += take;
            return take;
        }
        if (use_members) return members.read((char *)dst, n);
        const int r = gzread(gz, dst, (unsigned)std::min<size_t>(n, 1u << 30));
        if (r < 0) throw std::runtime_error("BAM file " + name + ": the gzip stream is corrupt");
        if ((size_t)r < n) {
            int err = 0;
            (void)gzerror(gz, &err);
            if (err != Z_OK && err != Z_STREAM_END) throw std::runtime_error("BAM file " + name + ": the gzip stream is corrupt or ends inside a block");
        }
        return (size_t)r;
    }
    // at least n (<= buf.size()) contiguous bytes at buf[pos], or false: the stream ends before
    bool need(size_t n)
    {
        if (len - pos >= n) return true;
        if (pos) { memmove(buf.data(), buf.data() + pos, len - pos); len -= pos; pos = 0; }
        while (len < n && !src_eof) {
            const size_t r = source_read(buf.data() + len, buf.size() - len);
            if (r == 0) src_eof = true;
            len += r;
        }
        return len >= n;
    }
    bool skip(uint64_t n)
    {
        while (n) {
            if (pos == len && !need(1)) return false;
            const size_t take = (size_t)std::min<uint64_t>(n, len - pos);
            pos += take;
            n -= take;
        }
        return true;
    }
    bool copy_to(char *dst, uint64_t n)
    {
        while (n) {
            if (pos == len && !need(1)) return false;
            const size_t take = (size_t)std::min<uint64_t>(n, len - pos);
            memcpy(dst, buf.data() + pos, take);
            dst += take;
            pos += take;
            n -= take;
        }
        return true;
    }
    static uint32_t le32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

    void read_header()
    {
        const char *ends = ": the stream ends inside the header";
        if (!need(4)) throw std::runtime_error("BAM file " + name + ends);
        if (memcmp(buf.data() + pos, "BAM\1", 4) != 0) throw std::runtime_error("BAM file " + name + ": wrong magic (the inflated stream does not begin with BAM\\1)");
        pos += 4;
        if (!need(4)) throw std::runtime_error("BAM file " + name + ends);
        const int32_t l_text = (int32_t)le32(buf.data() + pos);
        pos += 4;
        if (l_text < 0) throw std::runtime_error("BAM file " + name + ": negative l_text in the header");
        if (!skip((uint64_t)l_text)) throw std::runtime_error("BAM file " + name + ends);
        if (!need(4)) throw std::runtime_error("BAM file " + name + ends);
        const int32_t n_ref = (int32_t)le32(buf.data() + pos);
        pos += 4;
        if (n_ref < 0) throw std::runtime_error("BAM file " + name + ": negative n_ref in the header");
        for (int32_t i = 0; i < n_ref; ++i) {
            if (!need(4)) throw std::runtime_error("BAM file " + name + ends);
            const int32_t l_name = (int32_t)le32(buf.data() + pos);
            pos += 4;
            if (l_name < 0) throw std::runtime_error("BAM file " + name + ": negative l_name of reference " + std::to_string(i) + " in the header");
            if (!skip((uint64_t)l_name + 4)) throw std::runtime_error("BAM file " + name + ends);      // the name and l_ref
        }
    }

    // Appends the next selected record: its SEQ bytes to `seq` (each read starts on a byte boundary), its id to `ids`, and the byte
    // offset inside seq, the length in bases and the reverse byte to the three arrays.  false at the end of the stream.
    bool next(fastx::IdList &ids, fastx::BaseBuf &seq, std::vector<uint64_t> &off, std::vector<uint32_t> &rlen, std::vector<uint8_t> &rev)
    {
        for (;;) {
            if (!need(4)) {
                if (len == pos) return false;
                ++ordinal;
                fail("the stream ends inside the record (in block_size)");
            }
            ++ordinal;
            const uint64_t block_size = le32(buf.data() + pos);
            pos += 4;
            if (block_size < 32) fail("block_size " + std::to_string(block_size) + " is below the 32 bytes of the fixed fields");
            if (!need(32)) fail("the stream ends inside the record");
            const uint8_t *p = buf.data() + pos;
            const uint64_t l_read_name = p[8], n_cigar_op = p[12] | ((uint32_t)p[13] << 8);
            const uint32_t flag = p[14] | ((uint32_t)p[15] << 8);
            const uint32_t l_seq_u = le32(p + 16);
            pos += 32;
            if (l_seq_u >= (1u << 31)) fail("l_seq is negative or 2^31 and more (" + std::to_string((int32_t)l_seq_u) + ")");
            const uint64_t l_seq = l_seq_u, seq_bytes = (l_seq + 1) / 2;
            if (l_read_name == 0) fail("l_read_name is 0");
            const uint64_t fixed = 32 + l_read_name + 4 * n_cigar_op + seq_bytes + l_seq;
            if (block_size < fixed)
                fail("block_size " + std::to_string(block_size) + " is below 32 + l_read_name + 4*n_cigar_op + (l_seq+1)/2 + l_seq = " + std::to_string(fixed));
            if (!need((size_t)l_read_name)) fail("the stream ends inside the record (in read_name)");
            const char *nm = (const char *)buf.data() + pos;
            if (nm[l_read_name - 1] != '\0') fail("read_name is not NUL-terminated");
            const bool skipped = (flag & 0x900u) != 0;
            if (!skipped) {
                ids.data.append(nm, strlen(nm));
                ids.off.push_back(ids.data.size());
            }
            pos += (size_t)l_read_name;
            if (!skip(4 * n_cigar_op)) fail("the stream ends inside the record (in the CIGAR)");
            if (skipped) {
                ++n_skipped;
                if (!skip(block_size - 32 - l_read_name - 4 * n_cigar_op)) fail("the stream ends inside the record");
                continue;
            }
            const size_t at = seq.size();
            if (at + seq_bytes > seq.capacity()) {
                const size_t want = std::max<size_t>(at + seq_bytes, seq.capacity() + seq.capacity() / 2);
                if (grow) grow(want);
                seq.reserve(want);
            }
            seq.resize(at + seq_bytes);
            if (!copy_to(seq.data() + at, seq_bytes)) fail("the stream ends inside the record (in SEQ)");
            if (!skip(block_size - fixed + l_seq)) fail("the stream ends inside the record (in QUAL or the tags)");
            off.push_back(at);
            rlen.push_back((uint32_t)l_seq);
            rev.push_back((flag & 0x10u) ? 1 : 0);
            return true;
        }
    }

    [[noreturn]] void fail(const std::string &what) const
    {
        throw std::runtime_error("malformed BAM file " + name + ", record " + std::to_string(ordinal) + ": " + what);
    }
};

} // namespace bam
