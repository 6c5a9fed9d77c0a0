"""Search files larger than one range of `taxor profile`'s parser (taxor_amd/csrc/profile_cmd.h), as bytes: the padding of
tests/test_gpu_profile_scale.py and tests/test_profile_args_cpu.py and where the parser's ranges begin.  Nothing here needs a
device, numpy or the package."""
import random
import string

MIB = 1 << 20
PAD_CHARS = string.ascii_letters + string.digits + " _.,:;|/#-+=()[]"


def padded(tsv_bytes, target_bytes, seed):
    """tsv_bytes with the header as it is, every other line's REFERENCE_NAME (column 3) replaced by printable text of a seeded
    length, and ` pad=...` after the read id of about a third of the lines; at least target_bytes long.  The lengths spread over
    three orders of magnitude, so that a cut at a fixed fraction of the file falls into lines at unrelated places."""
    rng = random.Random(seed)
    block = "".join(rng.choice(PAD_CHARS) for _ in range(8192))
    head, *body = tsv_bytes.decode().split("\n")
    body = [ln for ln in body if ln]
    weight = [10.0 ** rng.uniform(-3, 0) for _ in body]
    need = max(0, target_bytes - len(tsv_bytes))
    scale = need / sum(weight)
    out = [head]
    for ln, w in zip(body, weight):
        f = ln.split("\t")
        k = int(w * scale) + 1 + rng.randrange(40)
        at = rng.randrange(len(block))
        f[2] = (block[at:] + block * (k // len(block) + 1))[:k]
        if rng.random() < 0.35:
            at = rng.randrange(len(block) - 300)
            f[0] += " pad=" + block[at:at + rng.randrange(1, 300)]
        out.append("\t".join(f))
    data = ("\n".join(out) + "\n").encode()
    assert len(data) >= target_bytes
    return data


def nominal_ranges(size):
    return min(16, size // MIB + 1)


def range_starts(data, n_ranges):
    """where each of n_ranges parser ranges begins: the line start at or after size / n_ranges * t"""
    cut = [0]
    for t in range(1, n_ranges):
        p = max(cut[-1], len(data) // n_ranges * t)
        nl = data.find(b"\n", p)
        cut.append(nl + 1 if nl >= 0 else len(data))
    return cut


def lines_of(data):
    """(start offset, read id) of every line after the header; the read id ends at the first space"""
    out, p = [], data.index(b"\n") + 1
    while p < len(data):
        e = data.find(b"\n", p)
        e = len(data) if e < 0 else e
        if e > p:
            out.append((p, data[p:e].split(b"\t")[0].split(b" ")[0]))
        p = e + 1
    return out


def reads_across(data, n_ranges):
    """read ids with a line before and a line after the start of some range"""
    lines, across = lines_of(data), set()
    for c in range_starts(data, n_ranges)[1:]:
        across |= {i for p, i in lines if p < c} & {i for p, i in lines if p >= c}
    return across
