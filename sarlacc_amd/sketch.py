"""sequenceGroups: reference-free pre-groups of a read batch from k-mer sketches (include/sarlacc_amd.h "reference-free
pre-groups of a read batch", csrc/sketch.hip).  The reference's correction vignette names two sources of
the `groups` of umiGroup: a mapping (readGroups) or to "cluster reads together using software like vsearch"; this is
the second, by a written specification of its own, in three device calls: a one-permutation MinHash sketch per read,
links between reads that share sketch entries, connected components; groups.labels_csr turns the labels into groups.
With `identity` a fourth call stands between the links and the components: every link is checked by a banded alignment
of its two reads (csrc/links_verify.hip, rule 6a) and only those within the identity threshold stay."""
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import check
from .groups import labels_csr

K_RANGE, BUCKETS, WINDOW_RANGE = (5, 31), (16, 32, 64, 128, 256), (1, 64)
BANDWIDTH_RANGE = (0, 127)
PPM = 10 ** 6
EMPTY = np.uint64(2 ** 64 - 1)


def _integer(x, name, lo, hi):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, numbers.Integral) or not lo <= int(x) <= hi:
        raise ValueError("'%s' should be an integer in %d .. %d" % (name, lo, hi))
    return int(x)


def check_args(k, buckets, window=1, min_shared=1):
    """Everything that can be refused before a device is touched; returns the four integers."""
    k = _integer(k, "k", *K_RANGE)
    if isinstance(buckets, (bool, np.bool_)) or not isinstance(buckets, numbers.Integral) or int(buckets) not in BUCKETS:
        raise ValueError("'buckets' should be a power of two in 16 .. 256")
    window = _integer(window, "window", *WINDOW_RANGE)
    if isinstance(min_shared, (bool, np.bool_)) or not isinstance(min_shared, numbers.Integral) or not 1 <= int(min_shared) <= int(buckets):
        raise ValueError("'min_shared' should be an integer in 1 .. buckets")
    return k, int(buckets), window, int(min_shared)


def check_verify_args(identity, bandwidth=100):
    """What verify_links can refuse before a device is touched; returns (max_diff_ppm, bandwidth).  `identity` is a real
    number in (0, 1]; it becomes max_diff_ppm = int(round((1 - identity) * 10^6)), the only form in which it reaches
    the device."""
    if isinstance(identity, (bool, np.bool_)) or not isinstance(identity, numbers.Real) or not 0.0 < float(identity) <= 1.0:
        raise ValueError("'identity' should be a number in (0, 1]")
    max_diff_ppm = int(round((1.0 - float(identity)) * PPM))
    if not 0 <= max_diff_ppm < PPM:
        raise ValueError("'identity' should be a number in (0, 1] that leaves fewer than 10^6 differences per 10^6 bases")
    return max_diff_ppm, _integer(bandwidth, "bandwidth", *BANDWIDTH_RANGE)


def empty_result():
    return {"group": np.zeros(0, np.int32), "groups": (np.zeros(1, np.int64), np.zeros(0, np.int32)),
            "n.kmers": np.zeros(0, np.int32), "n.pairs": np.int64(0), "n.links": np.int64(0)}


def device_bases(reads):
    """(device bases, device offsets, n) of a resident.DeviceReads, used where they lie, or of a generics.Reads, uploaded."""
    from .resident import DevBuffer, DeviceReads
    if isinstance(reads, DeviceReads):
        return reads.seq, reads.off, len(reads)
    s = reads.seq
    return DevBuffer.from_numpy(s.chars[:max(s.total, 1)]), DevBuffer.from_numpy(s.off), len(s)


def sketch_reads(d_seq, d_off, n, k, buckets, canonical=True):
    """sarlacc_dev_sketch_reads: (device uint64[n * buckets] sketches, device int32[n] numbers of k-mers)."""
    from .resident import DevBuffer
    sk, nk = DevBuffer(8 * max(n * buckets, 1)), DevBuffer(4 * max(n, 1))
    check(_lib.lib().sarlacc_dev_sketch_reads(d_seq, d_off, n, k, buckets, 1 if canonical else 0, sk, nk, None))
    return sk, nk


def sketch_links(d_sketch, n, buckets, window, min_shared, capacity=None):
    """sarlacc_dev_sketch_links: (device uint64 links a << 32 | b ascending, distinct candidate pairs, links).  A first
    call with room for `capacity` links (default 8 n) also fills; only when there are more does a second call run."""
    from .resident import DevBuffer
    cap = max(8 * n, 1024) if capacity is None else int(capacity)
    npairs, nlinks = C.c_int64(0), C.c_int64(0)
    for _ in range(2):
        links = DevBuffer(8 * max(cap, 1))
        check(_lib.lib().sarlacc_dev_sketch_links(d_sketch, n, buckets, window, min_shared, links, cap, C.byref(npairs),
                                                  C.byref(nlinks), None))
        if nlinks.value <= cap:
            break
        cap = nlinks.value
    return links, npairs.value, nlinks.value


def components(d_links, n_links, n, d_nkmers=None):
    """sarlacc_dev_components: (device int32 labels, number of groups)."""
    from .resident import DevBuffer
    label, ng = DevBuffer(4 * max(n, 1)), C.c_int64(0)
    check(_lib.lib().sarlacc_dev_components(d_links, n_links, n, d_nkmers, label, C.byref(ng), None))
    return label, ng.value


def verify_links(d_seq, d_off, n, d_links, n_links, identity, bandwidth=100, both_strands=True):
    """sarlacc_dev_links_verify: (device uint64 links that pass, in input order; their number; device int32[n_links]
    distances, -1 where the link fails; device uint8[n_links] strands).  A link a -- b passes when the unit-cost edit
    distance of its reads inside the band |j - i| <= bandwidth -- the edit distance itself whenever that is at most
    `bandwidth` -- is at most (max_diff_ppm * max(la, lb)) // 10^6, for b as it stands (strand 0, tried first) or, with
    both_strands, reverse-complemented (strand 1).  Only upper-case A, C, G, T match, and only themselves."""
    from .resident import DevBuffer
    max_diff_ppm, bandwidth = check_verify_args(identity, bandwidth)
    kept, dist, strand = DevBuffer(8 * max(n_links, 1)), DevBuffer(4 * max(n_links, 1)), DevBuffer(max(n_links, 1))
    nkept = C.c_int64(0)
    check(_lib.lib().sarlacc_dev_links_verify(d_seq, d_off, n, d_links, n_links, bandwidth, max_diff_ppm, 1 if both_strands else 0,
                                              dist, strand, kept, C.byref(nkept), None))
    return kept, nkept.value, dist, strand


def sequence_groups(reads, k=13, buckets=64, window=8, min_shared=3, canonical=True, identity=None, bandwidth=100):
    """generics.sequenceGroups."""
    k, buckets, window, min_shared = check_args(k, buckets, window, min_shared)
    if identity is not None:
        check_verify_args(identity, bandwidth)
    if not hasattr(reads, "seq") or not hasattr(reads, "__len__"):
        raise ValueError("'reads' should be a resident.DeviceReads or a Reads")
    if len(reads) == 0:
        return dict(empty_result(), **({} if identity is None else {"n.verified": np.int64(0)}))
    d_seq, d_off, n = device_bases(reads)
    d_sketch, d_nk = sketch_reads(d_seq, d_off, n, k, buckets, canonical)
    d_links, npairs, nlinks = sketch_links(d_sketch, n, buckets, window, min_shared)
    verified, nkept = {}, nlinks                           # the links the components run over
    if identity is not None:
        d_links, nkept, _, _ = verify_links(d_seq, d_off, n, d_links, nlinks, identity, bandwidth, both_strands=bool(canonical))
        verified["n.verified"] = np.int64(nkept)
    d_label, _ = components(d_links, nkept, n, d_nk)
    return {"group": d_label.to_numpy(np.int32, n).copy(), "groups": labels_csr(d_label, n),
            "n.kmers": d_nk.to_numpy(np.int32, n).copy(), "n.pairs": np.int64(npairs), "n.links": np.int64(nlinks), **verified}
