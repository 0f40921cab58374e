"""The host side of the BGZF writer: sarlacc_bgzf_deflate_bound, the end-of-file block, and the zlib yardsticks the GPU
tests measure the device encoder against.  No device."""
import ctypes as C
import zlib

import pytest

from tests import bgzf_cases, bgzf_write_cases as W


def _bound(nbytes):
    from sarlacc_amd import _lib
    n, cap = C.c_int64(-1), C.c_int64(-1)
    rc = _lib.lib().sarlacc_bgzf_deflate_bound(nbytes, C.byref(n), C.byref(cap))
    return rc, n.value, cap.value


@pytest.mark.parametrize("nbytes,blocks", [(0, 0), (1, 1), (65280, 1), (65281, 2), (2 ** 32 + 1, 65794)])
def test_bound(nbytes, blocks):
    from sarlacc_amd import bgzf
    rc, n, cap = _bound(nbytes)
    assert rc == 0 and n == blocks and cap >= blocks * 65536
    assert cap >= nbytes + 31 * blocks                 # what stored blocks need
    assert bgzf.deflate_bound(nbytes) == (n, cap)


def test_bound_refuses_a_negative_size():
    from sarlacc_amd import _lib, bgzf
    rc, _, _ = _bound(-1)
    assert rc != 0 and "negative" in _lib.lib().sarlacc_last_error().decode()
    with pytest.raises(_lib.SarlaccError, match="negative"):
        bgzf.deflate_bound(-5)


def test_eof_block():
    import gzip
    from sarlacc_amd import bgzf
    assert bgzf.EOF_BLOCK == bgzf_cases.EOF_BLOCK and len(bgzf.EOF_BLOCK) == 28
    assert gzip.decompress(bgzf.EOF_BLOCK) == b""


def test_yardsticks_reproduce_the_measured_ratios():
    """The figures the GPU size tests rest on, from zlib alone on the seeded text (8 blocks a read length): compressed
    bytes / text bytes of level 6, Z_HUFFMAN_ONLY, and Z_HUFFMAN_ONLY with a deflate block per line."""
    n = 8 * W.BLOCK
    long, short = W.yardsticks(2000), W.yardsticks(100)
    assert len(W.seeded_text(2000)) == len(W.seeded_text(100)) == n
    assert abs(long["level6"] / n - 0.468) < 0.005 and abs(long["level1"] / n - 0.489) < 0.005
    assert abs(long["huffman"] / n - 0.488) < 0.005 and abs(long["per_line"] / n - 0.391) < 0.005
    assert abs(short["huffman"] / n - 0.551) < 0.005 and abs(short["per_line"] / n - 0.650) < 0.005
    # the room the device encoder has at 2 kb, and why it must not take per-line tables at 100 bases
    assert 0.82 < long["per_line"] / long["level6"] < 0.85
    assert short["per_line"] > 1.15 * short["huffman"]


def test_limiter_texts_need_the_limiters():
    """zlib's own Huffman-only encoder on the two limiter blocks: its literal code reaches 15 bits where the unlimited
    code is deeper, and its code-length code reaches 7 bits where the header's symbol counts want 8."""
    for counts, depth in ((W.fibonacci_bytes(), None), (W.deep_bytes(), 20)):
        text = W.spread(counts, 6)
        assert len(text) <= W.BLOCK and len(counts) == len(set(v for v, _ in counts))
        _, _, lit, dist = W.first_table(W.zlib_raw(text, 6, zlib.Z_HUFFMAN_ONLY))
        assert max(lit) <= 15
        if depth:      # (zlib closes its first deflate block after 32 767 symbols, so its own table saw half the counts)
            assert W.huffman_depth([c for _, c in counts] + [1]) == depth
    assert len(W.fibonacci_bytes()) == 22 and sum(c for _, c in W.fibonacci_bytes()) == 46367
    text = W.spread(W.clen_limiter_bytes(), 5)
    assert len(text) == 2 ** 15 - 1
    clens, used, lit, _ = W.first_table(W.zlib_raw(text, 6, zlib.Z_HUFFMAN_ONLY))
    want = {v: 15 - (c.bit_length() - 1) for v, c in W.clen_limiter_bytes()}
    assert all(lit[v] == want.get(v, 0) for v in range(256)) and lit[256] == 15
    assert W.huffman_depth(used) == 8 and max(clens) == 7
