"""Loader for libsarlacc_amd.so (HIP kernels + C ABI, include/sarlacc_amd.h).

There is deliberately no fallback: if the shared library is missing or no HIP
device is usable, every compute call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SARLACC_LIB_PATH") or os.path.join(_HERE, "libsarlacc_amd.so")   # override: experiment builds
_lib = None


class SarlaccError(RuntimeError):
    """Error raised by the native library; the message is the reference's own
    wherever the reference would have thrown (src/utils.cpp, src/reference_align.cpp ...)."""


def _preload_shared_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two
    copies of the HIP runtime in one process cannot both own the GPU ("No HIP GPUs are
    available" in whichever initialises second), so when torch is installed its copy is loaded
    first and libsarlacc_amd.so binds to it by SONAME -- whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _try_build():
    """Build the in-tree library when it is missing and hipcc is available (fresh checkout)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        return
    try:
        subprocess.run(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc"), "HIPCC=" + hipcc],
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except subprocess.CalledProcessError as e:
        tail = (e.stdout or b"").decode(errors="replace")[-2000:]
        raise ImportError("sarlacc_amd: building %s failed (make exit %d):\n%s" % (LIB_PATH, e.returncode, tail))
    except OSError as e:
        raise ImportError("sarlacc_amd: cannot run make to build %s: %s" % (LIB_PATH, e))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            _try_build()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "sarlacc_amd: %s not found -- build it with `make -C sarlacc_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        _preload_shared_hip_runtime()
        _lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _lib


def check(rc):
    if rc:
        raise SarlaccError(lib().sarlacc_last_error().decode())


class Pointer(C.c_void_p):
    """The type of every pointer parameter of the C ABI, `void* stream` and `void** p` included.  Takes a numpy array
    (its data), a torch tensor (its data_ptr()), a resident.DevBuffer (through its _as_parameter_) and what c_void_p
    takes: None, bytes, a raw integer address, a c_void_p, a byref(...) result, a ctypes buffer."""

    @classmethod
    def from_param(cls, x):
        if isinstance(x, np.ndarray):
            return C.c_void_p(x.ctypes.data)
        if hasattr(x, "data_ptr"):
            return C.c_void_p(x.data_ptr())
        return C.c_void_p.from_param(x)


def _prototypes():
    """name -> (restype, [argtypes]) of every function include/sarlacc_amd.h declares, in its order
    (tests/test_abi_table.py holds the two together)."""
    i, i32, i64, u64, f64, s, p = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_char_p, Pointer
    reads = [p, p, p, p, i64]                 # seq, seq_off, qual, qual_off, n (umi_group: umi1, off1, umi2, off2, n)
    enc = [p, p, i]                           # enc_errors, enc_names, enc_n
    scored = reads + enc + [f64, f64, p, i]   # ... gapopen, gapext, reference, reference_len
    dev_align = [i64, i32] + enc + [f64, f64, p, i, i, p, p, i, p, p, p, p, p, p]
    msa_scores = [f64, f64, f64, f64, i]      # match, mismatch, gap_extension, gap_opening, bandwidth
    fused_tail = msa_scores + [f64, f64] + enc + [p, p, p, i64]
    clusters = [p, p, p]                      # nclusters, clu_off, clu
    return {
        "sarlacc_last_error": (s, []),
        "sarlacc_version": (i, []),
        "sarlacc_device_count": (i, []),
        "sarlacc_set_device": (i, [i]),
        "sarlacc_release_workspace": (None, []),
        "sarlacc_release_umi_workspace": (i64, []),
        "sarlacc_workspace_report": (i64, [p, i64]),
        "sarlacc_stage_ms": (f64, [s]),
        "sarlacc_stage_count": (f64, [s]),
        "sarlacc_last_kernel_ms": (f64, []),
        "sarlacc_align_locate_records": (i, [p, i64]),
        "sarlacc_adaptor_align": (i, scored + [p, p, i, p, p, p, p, p]),
        "sarlacc_adaptor_align_score_only": (i, scored + [p]),
        "sarlacc_barcode_align": (i, scored + [p]),
        "sarlacc_general_align": (i, scored + [i, p, p, p, p, p, i64]),
        "sarlacc_mask_bad_bases": (i, reads + enc + [f64, p]),
        "sarlacc_dev_align": (i, [p, p, p] + dev_align),
        "sarlacc_dev_pack_reads": (i, [p, i64, p, p, p]),
        "sarlacc_dev_align_packed": (i, [p, p, p, p] + dev_align),
        "sarlacc_dev_barcode_panel": (i, [p, p, p, i64, i32] + enc + [f64, f64, p, p, i, p, p, p, p, p]),
        "sarlacc_barcode_panel": (i, reads + enc + [f64, f64, p, p, i, p, p, p, p]),
        "sarlacc_dev_malloc": (i, [p, i64]),
        "sarlacc_dev_free": (i, [p]),
        "sarlacc_dev_pool_release": (i, []),
        "sarlacc_dev_upload": (i, [p, p, i64]),
        "sarlacc_dev_download": (i, [p, p, i64]),
        "sarlacc_host_alloc": (i, [p, i64]),
        "sarlacc_host_free": (i, [p]),
        "sarlacc_host_release": (i, []),
        "sarlacc_dev_windows": (i, [p, p, p, i64, p, i, p, p, p]),
        "sarlacc_dev_choose_strand": (i, [p, p, p, p, i64, i, i, p, p, p, p]),
        "sarlacc_dev_subseq": (i, [p, p, p, p, p, p, p, i64, p, i64, p, p]),
        "sarlacc_dev_realize": (i, [p, p, p, p, p, p, i64, p, p, p, p]),
        "sarlacc_dev_scramble": (i, [p, p, p, i64, u64, p, p, p]),
        "sarlacc_unmask_alignment": (i, [p, p, i64, p, p, i64, p]),
        "sarlacc_find_homopolymers": (i, [p, p, i64, p, p, p, p, i64, p]),
        "sarlacc_match_homopolymers": (i, [p, p, i64, p, p, i64, p, p, p, i64, p]),
        "sarlacc_find_errors": (i, [p, p, i64, p, p, i64, p, p, p, p, p, p, p, i64, p, p, i64, p]),
        "sarlacc_dev_profile_reads": (i, [p, p, p, i64, i32] + enc + [f64, f64, p, i, p, p, p, p, p, p]),
        "sarlacc_profile_fetch": (i, [p, p, p, p, i64, p, p, p, i64, p, p, p, i64]),
        "sarlacc_profile_reads": (i, scored + [p, p, p, p, p]),
        "sarlacc_dev_fastq_index": (i, [p, i64, p, p, p, p]),
        "sarlacc_dev_fastq_split": (i, [p, i64, i64, p, p, p]),
        "sarlacc_dev_fastq_extract": (i, [p, p, p, p, p, p, p]),
        "sarlacc_dev_fastq_format_size": (i, [p, i64, p, p, i64, p, p, p]),
        "sarlacc_dev_fastq_format": (i, [p, p, p, p, p, i64, p, i64, i64, p, p]),
        "sarlacc_dev_bam_format_size": (i, [p, p, p, i64, p, p, i64, p, p, p, p]),
        "sarlacc_dev_bam_format": (i, [p, p, p, p, p, i64, p, i64, i64, p, p]),
        "sarlacc_dev_bam_format_size_aux": (i, [p, p, p, i64, p, p, i64, p, p, p, p, p, p]),
        "sarlacc_dev_bam_format_aux": (i, [p, p, p, p, p, i64, p, p, p, i64, i64, p, p]),
        "sarlacc_dev_bam_tags_find": (i, [p, p, i64, p, p, p, p, p, p, p, p, p]),
        "sarlacc_dev_bam_tags_strings": (i, [p, p, i64, p, p, p, p, p, p, p]),
        "sarlacc_dev_bam_tags_ints": (i, [p, p, i64, p, p, p, p, p, p]),
        "sarlacc_dev_bam_tags_splice": (i, [p, p, i64, p, i64, p, p, p, i, p, p, p, p, p, p, p]),
        "sarlacc_dev_names_match": (i, [p, p, i64, p, p, i64, p, p, p]),
        "sarlacc_dev_records_pick": (i, [p, p, i64, i64, p, p, p]),
        "sarlacc_dev_locus_labels": (i, [p, p, p, p, i64, p, i64, i64, i, p, p, p]),
        "sarlacc_dev_labels_csr": (i, [p, i64, p, p, p, p, p]),
        "sarlacc_dev_sketch_reads": (i, [p, p, i64, i, i, i, p, p, p]),
        "sarlacc_dev_sketch_links": (i, [p, i64, i, i, i, p, i64, p, p, p]),
        "sarlacc_dev_links_verify": (i, [p, p, i64, p, i64, i, i64, i, p, p, p, p, p]),
        "sarlacc_dev_components": (i, [p, i64, i64, p, p, p, p]),
        "sarlacc_dev_sketch_candidates": (i, [p, i64, p, i64, i, i, i, p, p, p, p, p]),
        "sarlacc_dev_candidates_assign": (i, [p, p, i64, p, p, i64, p, p, i, i, i64, i, p, p, p, p, p, p, p, p]),
        "sarlacc_dev_sam_index": (i, [p, i64, i64, p, p, i64, p, p, p, i64, i, i64, p, p, p, p]),
        "sarlacc_dev_sam_extract": (i, [p, p, p, p, p, p, p, p, p, p]),
        "sarlacc_dev_bam_index": (i, [p, i64, i64, i, i64, p, i, i64, p, p, p, p, p]),
        "sarlacc_dev_bam_extract": (i, [p, p, p, p, p, p, p, p, p, p]),
        "sarlacc_bam_tile_bytes": (i, []),
        "sarlacc_dev_bam_reads_index": (i, [p, i64, i64, i, i, p, p, p, p]),
        "sarlacc_dev_bam_reads_range": (i, [i64, i64, p, p, p]),
        "sarlacc_dev_bam_reads_records": (i, [i64, p]),
        "sarlacc_dev_bam_reads_extract": (i, [p, i64, i64, i, p, p, p, p, p, p]),
        "sarlacc_dev_bam_reads_aux_range": (i, [i64, i64, p]),
        "sarlacc_dev_bam_reads_aux_extract": (i, [p, i64, i64, p, p, p]),
        "sarlacc_bgzf_scan": (i, [p, i64, i64, i64, p, p, p, p, p]),
        "sarlacc_dev_bgzf_inflate": (i, [p, p, p, i64, i64, p, i, p]),
        "sarlacc_bgzf_deflate_bound": (i, [i64, p, p]),
        "sarlacc_dev_bgzf_deflate": (i, [p, i64, i, p, i64, p, p, p]),
        "sarlacc_dev_bgzf_deflate_cuts": (i, [p, i64, p, i64, i64, i, p, i64, p, p, p]),
        "sarlacc_dev_copy": (i, [p, p, i64, p]),
        "sarlacc_dev_rfind_byte": (i, [p, i64, i, p, p]),
        "sarlacc_compute_lev_masked": (i, [p, p, i64, p]),
        "sarlacc_fast_levdist_test": (i, [p, p, i64, i, p, p, i64, p]),
        "sarlacc_cluster_umis_test": (i, [p, p, i64] + clusters),
        "sarlacc_umi_group": (i, reads + [i, i, p, p, i64] + clusters),
        "sarlacc_umi_pairs_shard": (i, [p, p, i64, i, i, i, p, i64, p]),
        "sarlacc_umi_group_from_pairs": (i, [p, p, i64, i, p, i64] + clusters),
        "sarlacc_dev_umi_pairs_shard": (i, [p, p, i64, i, i, i, p]),
        "sarlacc_dev_umi_pairs_fetch": (i, [p, i64]),
        "sarlacc_dev_umi_group_from_pairs": (i, [p, p, i64, i, p, i64] + clusters),
        "sarlacc_set_msa_spec": (i, [i]),
        "sarlacc_set_option": (i, [s, i]),
        "sarlacc_quick_msa": (i, [p, p, i64, p, p, i64] + msa_scores + [p, p, p, i64]),
        "sarlacc_create_consensus_basic_loop": (i, [p, p, p, i64, f64, f64, p, p, p, p]),
        "sarlacc_create_consensus_quality_loop": (i, [p, p, p, i64, p, p, p, f64] + enc + [p, p, p, p]),
        "sarlacc_msa_consensus": (i, [p, p, i64, p, p, p, p, i64] + fused_tail),
        "sarlacc_dev_msa_consensus": (i, [p, p, i64, p, p, p, i64] + fused_tail),
    }


PROTOTYPES = _prototypes()


ptr = Pointer.from_param   # (no call in the package needs it any more; tools/perf_sam.py names it)


class _HostBlock:
    """A page-locked block of sarlacc_host_alloc behind the array interface; goes back to the library's pool with its last view."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib().sarlacc_host_alloc(C.byref(p), nbytes))
        self.address = p.value
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (self.address, False), "version": 3}

    def __del__(self):
        try:
            if self.address:
                lib().sarlacc_host_free(self.address)
                self.address = 0
        except Exception:
            pass


_DEBUG_ZERO = os.environ.get("SARLACC_DEBUG_ZERO_HOST") == "1"


def host_array(count, dtype):
    """Uninitialised numpy array for a result the device writes in full: page-locked from 1 MB on (sarlacc_host_alloc: the
    download is one DMA transfer instead of a staged copy), ordinary memory below that.  Contents beyond what the C call
    wrote are UNDEFINED (a pooled block keeps what its last user left): callers read only the range the call reports
    (offsets[-1] of a string set, the returned count); SARLACC_DEBUG_ZERO_HOST=1 zero-fills for debugging."""
    dt = np.dtype(dtype)
    nbytes = int(count) * dt.itemsize
    if nbytes < (1 << 20):
        return np.zeros(int(count), dt) if _DEBUG_ZERO else np.empty(int(count), dt)
    arr = np.asarray(_HostBlock(nbytes))[:nbytes].view(dt)
    if _DEBUG_ZERO:
        arr[:] = 0
    return arr


def device_count():
    return int(lib().sarlacc_device_count())


def set_device(device):
    check(lib().sarlacc_set_device(int(device)))


def release_umi_workspace():
    """sarlacc_release_umi_workspace: gives the umi_group stage's cached device buffers back (bytes freed)."""
    return int(lib().sarlacc_release_umi_workspace())


def workspace_report(top=12):
    """sarlacc_workspace_report: (total bytes, [(name, bytes), ...] of the `top` largest cached device buffers)."""
    buf = C.create_string_buffer(1 << 16)
    total = int(lib().sarlacc_workspace_report(buf, len(buf)))
    rows = [ln.rsplit(" ", 1) for ln in buf.value.decode().splitlines() if ln]
    return total, [(n, int(b)) for n, b in rows[:top]]


def stage_ms(name):
    """Milliseconds of the named kernel group in the last call that ran it (HIP events), <0 if none."""
    return float(lib().sarlacc_stage_ms(name.encode()))


def stage_count(name):
    """Work counter (cells, pairs ...) recorded by the last call that set it, <0 if unset."""
    return float(lib().sarlacc_stage_count(name.encode()))


def last_kernel_ms():
    return float(lib().sarlacc_last_kernel_ms())


def align_locate_records(n):
    """{I_max, lo, hi} per read as the locator of the last adaptor-align call reported them (n x 3 int32; diagnostic)."""
    out = np.zeros((int(n), 3), dtype=np.int32)
    check(lib().sarlacc_align_locate_records(out, int(n)))
    return out
