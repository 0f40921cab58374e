"""referenceGroups: resident reads assigned to the references they were made from (include/sarlacc_amd.h "resident reads
assigned to references", csrc/ref_map.hip).  The reference's correction vignette builds the `groups` of
umiGroup from a mapping to a transcriptome, and its profiling vignette the reference of every read; both send the reads
to an outside mapper and read its SAM back (sam2ranges, readGroups).  Here the expected sequences are sketched like the
reads (sketch.sketch_reads) and two device calls follow: the join of read sketches against reference sketches into a
bounded candidate list per read, and the check of every candidate by the banded alignment of sequenceGroups' rule 6a
with the choice of one reference per read; groups.labels_csr turns the chosen references into groups."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .groups import labels_csr
from .sketch import _integer, check_args, check_verify_args, device_bases, sketch_reads

MAX_CANDIDATES_RANGE = (1, 16)


def check_reference_args(k, buckets, min_shared, max_candidates, identity, bandwidth):
    """Everything that can be refused before a device is touched; returns (k, buckets, min_shared, max_candidates,
    max_diff_ppm or -1 for no check, bandwidth)."""
    k, buckets, _, min_shared = check_args(k, buckets, 1, min_shared)
    max_candidates = _integer(max_candidates, "max_candidates", *MAX_CANDIDATES_RANGE)
    max_diff_ppm, bandwidth = (-1, _integer(bandwidth, "bandwidth", 0, 127)) if identity is None else check_verify_args(identity, bandwidth)
    return k, buckets, min_shared, max_candidates, max_diff_ppm, bandwidth


def as_references(references):
    """A list of strings (upper-cased), a generics.Reads or a resident.DeviceReads -> something device_bases takes."""
    from .generics import Reads
    if hasattr(references, "seq") and hasattr(references, "__len__"):
        return references
    if isinstance(references, (str, bytes)) or not all(isinstance(s, str) for s in references):
        raise ValueError("'references' should be a list of strings, a Reads or a resident.DeviceReads")
    return Reads([s.upper() for s in references])


def result_without_device(n_reads, n_refs, checked):
    """No reads or no references: no read has a reference and nothing was sketched, so the k-mer counts are -1."""
    minus = np.full(n_reads, -1, np.int32)
    out = {"reference": minus, "strand": np.zeros(n_reads, np.uint8), "dist": minus.copy(), "shared": np.zeros(n_reads, np.int32),
           "n.candidates": np.zeros(n_reads, np.int32), "n.kmers": minus.copy(), "ref.n.kmers": np.full(n_refs, -1, np.int32),
           "group": minus.copy(), "groups": (np.zeros(1, np.int64), np.zeros(0, np.int32)), "n.hits": np.int64(0)}
    if checked:
        out["n.checked"] = np.int64(0)
    return out


def sketch_candidates(d_ref_sketch, n_refs, d_read_sketch, n_reads, buckets, min_shared, max_candidates):
    """sarlacc_dev_sketch_candidates: (device int32[n_reads * max_candidates] references, the same of `shared`, device
    int32[n_reads] numbers of candidates, hits)."""
    from .resident import DevBuffer
    slots = 4 * max(n_reads * max_candidates, 1)
    cand_ref, cand_shared, ncand, nhits = DevBuffer(slots), DevBuffer(slots), DevBuffer(4 * max(n_reads, 1)), C.c_int64(0)
    check(_lib.lib().sarlacc_dev_sketch_candidates(d_ref_sketch, n_refs, d_read_sketch, n_reads, buckets, min_shared, max_candidates,
                                                   cand_ref, cand_shared, ncand, C.byref(nhits), None))
    return cand_ref, cand_shared, ncand, nhits.value


def candidates_assign(d_ref_seq, d_ref_off, n_refs, d_read_seq, d_read_off, n_reads, d_cand_ref, d_cand_shared, max_candidates,
                      bandwidth=100, max_diff_ppm=-1, both_strands=True, per_slot=False):
    """sarlacc_dev_candidates_assign: ((device reference, strand, dist, shared per read), candidates checked), and with
    per_slot also (device int32 dist, device uint8 strand) of every slot."""
    from .resident import DevBuffer
    n = max(n_reads, 1)
    out = DevBuffer(4 * n), DevBuffer(n), DevBuffer(4 * n), DevBuffer(4 * n)
    slot = (DevBuffer(4 * n * max_candidates), DevBuffer(n * max_candidates)) if per_slot else (None, None)
    nchecked = C.c_int64(0)
    check(_lib.lib().sarlacc_dev_candidates_assign(d_ref_seq, d_ref_off, n_refs, d_read_seq, d_read_off, n_reads, d_cand_ref, d_cand_shared,
                                                   max_candidates, bandwidth, max_diff_ppm, 1 if both_strands else 0, *out, *slot,
                                                   C.byref(nchecked), None))
    return (out, nchecked.value, slot) if per_slot else (out, nchecked.value)


def reference_groups(reads, references, k=13, buckets=64, min_shared=2, max_candidates=4, identity=0.8, bandwidth=100, both_strands=True):
    """generics.referenceGroups."""
    k, buckets, min_shared, max_candidates, max_diff_ppm, bandwidth = check_reference_args(k, buckets, min_shared, max_candidates,
                                                                                          identity, bandwidth)
    if not hasattr(reads, "seq") or not hasattr(reads, "__len__"):
        raise ValueError("'reads' should be a resident.DeviceReads or a Reads")
    references = as_references(references)
    n, nf, both = len(reads), len(references), bool(both_strands)
    if n == 0 or nf == 0:
        return result_without_device(n, nf, identity is not None)
    d_seq, d_off, _ = device_bases(reads)
    d_fseq, d_foff, _ = device_bases(references)
    d_fsketch, d_fnk = sketch_reads(d_fseq, d_foff, nf, k, buckets, both)
    d_sketch, d_nk = sketch_reads(d_seq, d_off, n, k, buckets, both)
    d_cand_ref, d_cand_shared, d_ncand, nhits = sketch_candidates(d_fsketch, nf, d_sketch, n, buckets, min_shared, max_candidates)
    (d_reference, d_strand, d_dist, d_shared), nchecked = candidates_assign(d_fseq, d_foff, nf, d_seq, d_off, n, d_cand_ref, d_cand_shared,
                                                                           max_candidates, bandwidth, max_diff_ppm, both)
    reference = d_reference.to_numpy(np.int32, n).copy()
    out = {"reference": reference, "strand": d_strand.to_numpy(np.uint8, n).copy(), "dist": d_dist.to_numpy(np.int32, n).copy(),
           "shared": d_shared.to_numpy(np.int32, n).copy(), "n.candidates": d_ncand.to_numpy(np.int32, n).copy(),
           "n.kmers": d_nk.to_numpy(np.int32, n).copy(), "ref.n.kmers": d_fnk.to_numpy(np.int32, nf).copy(),
           "group": reference.copy(), "groups": labels_csr(d_reference, n), "n.hits": np.int64(nhits)}
    if identity is not None:
        out["n.checked"] = np.int64(nchecked)
    return out
