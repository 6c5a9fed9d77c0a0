"""The CPU restatement of census_format.h (taxor_amd/csrc): the key estimate of a bin from its column's nonzero bytes, an IXF's capacity,
the sums per user bin and IXF and the text of `taxor census`'s two files and of the columns `--coverage-breadth` appends.  Everything
is computed from the host layout's own bytes with numpy; nothing here calls the library.  Shared by the census tests."""
import math

import numpy as np

REF_COLUMNS = "#ACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tLEAF_BINS\tINDEX_HASHES\tHASHES_PER_KB\n"
IXF_COLUMNS = "#IXF\tBINS\tLEAF_BINS\tMERGED_BINS\tROWS\tCAPACITY\tMAX_BIN_KEYS\tFILL\tBYTES\n"
BREADTH_COLUMNS = "\tINDEX_HASHES\tBREADTH\tEXPECTED_BREADTH\tBREADTH_RATIO"


def llround(x):
    """C's llround for x >= 0: halves away from zero"""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def keys_est(nonzero):
    return llround(float(int(nonzero)) * 256.0 / 255.0)


def seg_len_of(n):
    """taxor_ixf_seg_len: (size_t)(32 + 1.23 * n) / 3"""
    return int(32 + 1.23 * float(n)) // 3


def capacity(seg_len):
    """the largest n with seg_len_of(n) <= seg_len, by walking from the real-valued solution; 0 when none fits"""
    if seg_len_of(0) > seg_len:
        return 0
    n = max(0, int((3 * seg_len - 32) / 1.23) - 4)
    while seg_len_of(n) > seg_len:
        n -= 1
    while seg_len_of(n + 1) <= seg_len:
        n += 1
    return n


def bound(n):
    """five standard deviations of Binomial(n, 255/256) scaled by 256/255, plus the rounding: derived, not measured"""
    return 5.0 * math.sqrt(n / 255.0) + 1.0


def nonzero_of(host):
    """per IXF the nonzero bytes of every bin's column (padding columns left out), from the host bytes"""
    return [np.count_nonzero(np.asarray(f["data"], np.uint8).reshape(3 * f["seg_len"], f["stride"])[:, :f["bins"]], axis=0).astype(np.uint64) for f in host]


class Census:
    """nonzero: per IXF a uint64 array [bins]; shapes: the IXF dicts (bins, stride, seg_len, fname_idx)"""

    def __init__(self, shapes, nonzero, n_user_bins):
        self.index_hashes = [0] * n_user_bins          # None = NA
        self.leaf_bins = [0] * n_user_bins
        self.ixf = []                                  # (bins, leaf_bins, seg_len, stride, capacity, max_bin_keys or None)
        for f, nz in zip(shapes, nonzero):
            cap = capacity(f["seg_len"])
            leaves, mx = 0, 0
            for j in range(f["bins"]):
                peeled = int(nz[j]) <= cap
                est = keys_est(nz[j])
                if not peeled:
                    mx = None
                elif mx is not None:
                    mx = max(mx, est)
                b = int(f["fname_idx"][j])
                if b < 0:
                    continue
                leaves += 1
                self.leaf_bins[b] += 1
                if not peeled:
                    self.index_hashes[b] = None
                elif self.index_hashes[b] is not None:
                    self.index_hashes[b] += est
            self.ixf.append((f["bins"], leaves, f["seg_len"], f["stride"], cap, mx))

    def refs_text(self, sp):
        by_bin = {}
        for s in sp:
            by_bin.setdefault(s["user_bin"], s)
        out = REF_COLUMNS
        for b, ih in enumerate(self.index_hashes):
            s = by_bin.get(b, sp[0])
            out += ref_line(s["accession_id"], s["organism_name"], s["taxid"], s["seq_len"], self.leaf_bins[b], ih)
        return out

    def ixfs_text(self):
        return IXF_COLUMNS + "".join(ixf_line(x, bins, leaves, seg, stride, mx) for x, (bins, leaves, seg, stride, _, mx) in enumerate(self.ixf))


def ref_line(accession, name, taxid, ref_len, leaf_bins, index_hashes):
    per_kb = "NA" if index_hashes is None or ref_len == 0 else "%.2f" % (float(index_hashes) * 1000.0 / float(ref_len))
    return "\t".join([accession, name, taxid, str(ref_len), str(leaf_bins), "NA" if index_hashes is None else str(index_hashes), per_kb]) + "\n"


def ixf_line(x, bins, leaf_bins, seg_len, stride, max_bin_keys):
    cap = capacity(seg_len)
    fill = "NA" if max_bin_keys is None or cap == 0 else "%.3f" % (float(max_bin_keys) / float(cap))
    return "\t".join(str(v) for v in [x, bins, leaf_bins, bins - leaf_bins, 3 * seg_len, cap, "NA" if max_bin_keys is None else max_bin_keys, fill,
                                      3 * seg_len * stride]) + "\n"


def breadth_columns(distinct, hash_matches, index_hashes):
    if index_hashes is None:
        return "\tNA\tNA\tNA\tNA"
    if index_hashes == 0:
        return "\t0\tNA\tNA\tNA"
    ih = float(index_hashes)
    breadth = min(1.0, float(distinct) / ih)
    expected = 1.0 - math.exp(-float(hash_matches) / ih)
    e = "%.4f" % expected
    return "\t%d\t%.4f\t%s\t%s" % (index_hashes, breadth, e, "NA" if e == "0.0000" else "%.2f" % (breadth / expected))
