"""Device-resident entry points (sarlacc_dev_* of include/sarlacc_amd.h): inputs and
outputs are raw device pointers (e.g. torch tensors' data_ptr()), work is enqueued on
the caller's HIP stream.  Used by bench.py and by pipelines that keep reads in HBM."""
import numpy as np

from . import _lib
from ._lib import check
from .calls import _csr_args, _fused_consensus
from .encoding import as_encoding


def dev_pack_reads(d_seq, total, d_packed, d_nmask, stream=0):
    """sarlacc_dev_pack_reads: ASCII bases -> 2-bit packed bases + exception bit-mask (both on device)."""
    check(_lib.lib().sarlacc_dev_pack_reads(d_seq, int(total), d_packed, d_nmask, stream))


def dev_align(d_seq, d_qual, d_off, n, max_len, encoding, gapopen, gapext, reference, local=True,
              sec_starts=(), sec_ends=(), d_scores=None, d_starts=None, d_ends=None,
              d_sec_start=None, d_sec_width=None, stream=0, d_nmask=None):
    """sarlacc_dev_align(_packed): quality-weighted DP of `reference` against n device-resident reads.
    With d_starts/d_ends given the traceback (adaptor_align) variant runs, else scores only.
    With d_nmask given, d_seq holds 2-bit packed bases (dev_pack_reads)."""
    enc = as_encoding(encoding)
    rf = reference.encode() if isinstance(reference, str) else bytes(reference)
    ss = np.ascontiguousarray(sec_starts, dtype=np.int32).reshape(-1)
    se = np.ascontiguousarray(sec_ends, dtype=np.int32).reshape(-1)
    ns = ss.size
    if ns == 0:
        ss = np.zeros(1, np.int32)
        se = np.zeros(1, np.int32)
    args = (d_qual, d_off, int(n), int(max_len), enc.errors, enc.names, len(enc), gapopen, gapext,
            rf, len(rf), 0 if local else 1, ss, se, ns, d_scores, d_starts, d_ends, d_sec_start, d_sec_width, stream)
    if d_nmask is not None:
        check(_lib.lib().sarlacc_dev_align_packed(d_seq, d_nmask, *args))
    else:
        check(_lib.lib().sarlacc_dev_align(d_seq, *args))


def dev_msa_consensus(grp_off, grp, d_seq, d_qual, off_host, match, mismatch, gapExtension, gapOpening, bandwidth,
                      min_cov, pseudo_count=1.0, encoding=None):
    """sarlacc_dev_msa_consensus: multiReadAlign + consensusReadSeq on reads (and qualities) already in
    HBM.  `off_host` is the host copy (numpy int64[n+1]) of the read offsets, grp_off/grp the CSR of
    1-based group lists.  d_qual None -> basic vote.  Returns (consensus StringSet, phred StringSet)."""
    goff, gvals = _csr_args(grp_off, grp)
    off = np.ascontiguousarray(off_host, dtype=np.int64)
    enc = as_encoding(encoding) if d_qual is not None else None
    # (page-locked results: 360 MB come back at a 10^6-read pass)
    return _fused_consensus(_lib.lib().sarlacc_dev_msa_consensus, goff, gvals, (d_seq, d_qual, off, off.size - 1), np.diff(off),
                            (match, mismatch, gapExtension, gapOpening, int(bandwidth), min_cov, pseudo_count), enc, _lib.host_array)
