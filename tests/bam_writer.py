"""BAM files for the tests, written with the standard library only (SAMv1 sections 4.1 and 4.2 restated: neither samtools nor
pysam is at hand, so this helper is the only pin of the format).  BGZF framing by hand: gzip member with the extra subfield
'B' 'C' (SLEN 2, BSIZE = block length - 1), raw deflate, CRC-32, ISIZE, and the 28-byte end-of-file block.

A read is (name: bytes, codes: sequence of nibbles 0..15, flag: int).  `restored` decodes one back to the ASCII read a FASTQ
converter with `samtools fastq`'s defaults would write: the letters of the nibbles, and for flag 0x10 the reverse complement taken
on the IUPAC codes.  That decoding is the expected value of every BAM test."""
import struct
import zlib

import numpy as np

ALPHABET = b"=ACMGRSVTWYHKDBN"
# complement of an IUPAC code = its four bits reversed (A=1 <-> T=8, C=2 <-> G=4; M=3 <-> K=12, ...)
COMPLEMENT = [((n & 1) << 3) | ((n & 2) << 1) | ((n & 4) >> 1) | ((n & 8) >> 3) for n in range(16)]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data: bytes, level=6) -> bytes:
    assert len(data) < 65280
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = co.compress(data) + co.flush()
    total = 18 + len(cdata) + 8
    assert total <= 65536
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


assert bgzf_block(b"") == EOF_BLOCK


def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def seq_bytes(codes, spare=0):
    """4-bit SEQ field: two bases per byte, the first in the high nibble; `spare` fills the low nibble behind an odd length"""
    c = [int(x) for x in codes]
    if len(c) & 1:
        c.append(spare)
    return bytes((c[i] << 4) | c[i + 1] for i in range(0, len(c), 2))


def record(name, codes, flag=4, cigar=(), tags=b"", spare=0, ref_id=-1, pos=-1):
    """one alignment record, block_size in front (CIGAR ops as (length, op) pairs)"""
    nm = name + b"\0"
    assert 1 <= len(nm) <= 255
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), 0, 4680, len(cigar), flag, len(codes), -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", (n << 4) | op) for n, op in cigar)
    body += seq_bytes(codes, spare) + b"\xff" * len(codes) + tags
    return struct.pack("<I", len(body)) + body


def bgzf(stream: bytes, cuts=None, block=60000, eof=True) -> bytes:
    """the byte stream in BGZF blocks: cut at the offsets `cuts` (then no block may pass 65279 bytes) or every `block` bytes"""
    if cuts is None:
        cuts = list(range(block, len(stream), block))
    edges = [0] + [c for c in sorted(set(cuts)) if 0 < c < len(stream)] + [len(stream)]
    out = b"".join(bgzf_block(stream[a:b]) for a, b in zip(edges[:-1], edges[1:]) if b > a)
    return out + (EOF_BLOCK if eof else b"")


def write_bam(path, reads, blocking="bytes", block=60000, eof=True, head=None, spare=0, extras=None):
    """reads: [(name, codes, flag)].  blocking: "bytes" (blocks of `block` bytes: records straddle), "record" (the header and every
    record in a block of its own) or "one" (a single block).  extras: {read index: dict(cigar=..., tags=...)}"""
    head = header() if head is None else head
    recs = [record(n, c, f, spare=spare, **((extras or {}).get(i, {}))) for i, (n, c, f) in enumerate(reads)]
    stream = head + b"".join(recs)
    if blocking == "record":
        cuts, at = [], len(head)
        for r in recs:
            cuts.append(at)
            at += len(r)
        data = bgzf(stream, cuts=cuts, eof=eof)
    elif blocking == "one":
        data = bgzf(stream, cuts=[], eof=eof)
    else:
        data = bgzf(stream, block=block, eof=eof)
    with open(path, "wb") as f:
        f.write(data)
    return stream


def restored(codes, flag) -> bytes:
    c = [int(x) for x in codes]
    if flag & 0x10:
        c = [COMPLEMENT[x] for x in reversed(c)]
    return bytes(ALPHABET[x] for x in c)


def selected(reads):
    """[(id, restored ASCII read)] of the records `taxor search` takes: secondary and supplementary ones left out"""
    return [(n, restored(c, f)) for n, c, f in reads if not f & 0x900]


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for n, s in selected(reads):
            f.write(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def codes_of_ascii(seq: bytes):
    """ACGT... letters -> nibbles"""
    lut = np.zeros(256, np.uint8)
    for i, ch in enumerate(ALPHABET):
        lut[ch] = i
    return lut[np.frombuffer(seq, np.uint8)]
