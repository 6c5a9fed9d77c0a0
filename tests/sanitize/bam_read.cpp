// AddressSanitizer / UBSan driver for the BAM reader (bam.h):
//   bam_read <file>            -> "<records> records <bases> bases <skipped> skipped fnv <hash>" once through the parallel inflate and once
//                                 through the one zlib stream, or "error: <what>"
//   bam_read <file> truncate   -> the inflated stream cut at every byte up to the end of its second record, read from memory:
//                                 "<n> cuts: <clean> clean ends, <errors> errors"
#include "bam.h"
#include <cstdio>

static void run(bam::Reader &rd)
{
    fastx::IdList ids;
    fastx::BaseBuf seq;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> rev;
    uint64_t bases = 0, h = 1469598103934665603ull;
    std::string s;
    while (rd.next(ids, seq, off, len, rev)) {
        s.clear();
        bam::restore_read((const uint8_t *)seq.data() + off.back(), len.back(), rev.back() != 0, s);
        for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
        bases += len.back();
    }
    printf("%zu records %llu bases %llu skipped fnv %016llx\n", ids.size(), (unsigned long long)bases, (unsigned long long)rd.n_skipped, (unsigned long long)h);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (argc == 2) {
        for (int sequential = 0; sequential < 2; ++sequential) {
            try {
                if (bam::sniff(argv[1]) != bam::BAM) { puts("not BAM"); continue; }
                bam::Reader rd;
                rd.open(argv[1], 3, sequential != 0);
                run(rd);
            } catch (const std::exception &ex) { printf("error: %s\n", ex.what()); }
        }
        return 0;
    }
    std::vector<uint8_t> data;
    {
        gzFile f = gzopen(argv[1], "rb");
        if (!f) return 2;
        uint8_t tmp[1 << 16];
        int r;
        while ((r = gzread(f, tmp, sizeof tmp)) > 0) data.insert(data.end(), tmp, tmp + r);
        gzclose(f);
    }
    size_t limit = 0;
    {
        bam::Reader rd;
        rd.open_mem(data.data(), data.size());
        fastx::IdList ids;
        fastx::BaseBuf seq;
        std::vector<uint64_t> off;
        std::vector<uint32_t> len;
        std::vector<uint8_t> rev;
        rd.next(ids, seq, off, len, rev);
        rd.next(ids, seq, off, len, rev);
        limit = rd.mem_pos - (rd.len - rd.pos);
    }
    size_t clean = 0, errors = 0;
    for (size_t cut = 0; cut <= limit; ++cut) {
        std::vector<uint8_t> part(data.begin(), data.begin() + (long)cut);      // its own allocation: a read past the cut is a finding
        try {
            bam::Reader rd;
            rd.open_mem(part.data(), part.size());
            fastx::IdList ids;
            fastx::BaseBuf seq;
            std::vector<uint64_t> off;
            std::vector<uint32_t> len;
            std::vector<uint8_t> rev;
            while (rd.next(ids, seq, off, len, rev)) {}
            ++clean;
        } catch (const std::exception &) { ++errors; }
    }
    printf("%zu cuts: %zu clean ends, %zu errors\n", limit + 1, clean, errors);
    return 0;
}
