"""The small kernels every pipeline path runs through -- csrc/resident.hip (k_windows, k_realize, k_subseq, k_scramble,
k_choose_strand) and csrc/mask.hip (k_unmask, k_mask) -- compared byte for byte with tests/resident_cases.py, the plain
restatement that tests/test_resident_cases.py pins, with the host routes of the package and with the CPU oracle.
Everything is bytes, int32 and bit-compared fp64: no tolerance.

Every batch is uploaded at its exact size, once ending in a non-empty read and once in an empty one, and the quality
byte of position p is p & 0xff, so that a byte that moved shows.  The sizes sit around the kernels' workgroups (64, 128
and 256 threads, 64 columns per step of k_unmask); the grid-stride loops of k_unmask and k_mask are reached with sizes
taken from the device's number of compute units.  A bad argument is refused on the host and never reaches a kernel."""
import numpy as np
import pytest

from tests import resident_cases as R

pytestmark = pytest.mark.gpu


def _device_reads(seqs, quals):
    """A resident batch whose buffers are exactly as long as the reads."""
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    assert [len(q) for q in quals] == [len(s) for s in seqs]
    s, q = np.frombuffer(b"".join(seqs), np.uint8), np.frombuffer(b"".join(quals), np.uint8)
    return DeviceReads(DevBuffer.from_numpy(s), DevBuffer.from_numpy(q), DevBuffer.from_numpy(off), off, None)


def _strings(ss):
    return [ss.chars[ss.off[i]:ss.off[i + 1]].tobytes() for i in range(len(ss))]


def _download(dev):
    s, q = dev.download()
    return _strings(s), _strings(q)


def _differing(got, want):
    """The first few entries that differ, for the message of an assert."""
    return [(i, g[:40], w[:40]) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3] or (len(got), len(want))


def _same(got, want, what):
    for g, w, part in zip(got, want, ("bases", "qualities")):
        assert g == w, (what, part, _differing(g, w))


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- complement ---------------------------------------------------------------------------------------------------
def test_complement_of_every_byte():
    what, seqs, quals = R.complement_case()
    dev = _device_reads(seqs, quals)
    want = [R.revcomp(s) for s in seqs], [q[::-1] for q in quals]
    assert want[0][1] == R.COMPLEMENT[::-1].tobytes() and want[1][1] == bytes(range(255, -1, -1))
    _same(_download(dev.front_and_back(1000)[1]), want, what + ", back window")
    _same(_download(dev.realize([0, 1], [1, 1])), want, what + ", realize")
    _same(_download(dev.realize([1, 0], [0, 0])), (seqs[::-1], quals[::-1]), what + ", realize forward")


# ---- windows ------------------------------------------------------------------------------------------------------
def test_windows_at_every_length_and_tolerance():
    from sarlacc_amd import generics
    uploaded = {}
    for what, seqs, quals, tol in R.window_cases():
        key = (len(seqs), len(seqs[-1]) if seqs else -1)
        if key not in uploaded:
            uploaded[key] = _device_reads(seqs, quals), generics.Reads(seqs, quals)
        dev, host = uploaded[key]
        front, back = dev.front_and_back(tol)
        wf, wb = R.windows(seqs, quals, tol)
        _same(_download(front), wf, what + ", front")
        _same(_download(back), wb, what + ", back")
        hf, hb = generics._get_front_and_back(host, tol)
        _same(_download(front), (_strings(hf.seq), _strings(hf.qual)), what + ", front, host route")
        _same(_download(back), (_strings(hb.seq), _strings(hb.qual)), what + ", back, host route")
        assert len(front) == len(back) == len(seqs)


# ---- realize ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty_last", [False, True], ids=["last read not empty", "last read empty"])
def test_realize_orders_strands_and_trims(empty_last):
    seqs, quals = R.batch(R.REALIZE_LENGTHS, 102, empty_last)
    dev = _device_reads(seqs, quals)
    for what, idx, rev, ts, te in R.realize_cases():
        got = dev.realize(idx, rev, ts, te)
        _same(_download(got), R.realize(seqs, quals, idx, rev, ts, te), what)
        assert len(got) == len(idx)
    # on a reversed read [2, L] drops the original's last base and [1, L - 1] its first
    L = R.REALIZE_LENGTHS[8]
    got = _download(dev.realize([8, 8], [1, 1], [2, 1], [L, L - 1]))
    assert got[0] == [R.revcomp(seqs[8][:-1]), R.revcomp(seqs[8][1:])] and got[1] == [quals[8][:-1][::-1], quals[8][1:][::-1]]


# ---- subseq -------------------------------------------------------------------------------------------------------
def test_subseq_inside_the_reads():
    uploaded = {}
    for what, a, b, from_b, start, width in R.subseq_cases():
        for reads in (a, b):
            if reads is not None and tuple(reads) not in uploaded:
                uploaded[tuple(reads)] = _device_reads(reads, reads)
        da = uploaded[tuple(a)]
        if b is None:
            got = da.subseq(start, width)
        else:
            got = da.subseq(start, width, other=uploaded[tuple(b)], from_other=from_b)
        want = R.subseq(a, b, from_b, start, width)
        assert _strings(got) == want, (what, _differing(_strings(got), want))


def test_subseq_refuses_a_range_outside_its_read():
    from sarlacc_amd._lib import SarlaccError
    da = db = None
    for what, a, b, from_b, start, width, named in R.subseq_refusals():
        if da is None:
            da, db = _device_reads(a, a), _device_reads(b, b)
        with pytest.raises(SarlaccError, match="sub-sequence of read %d lies outside the read$" % (named + 1)):
            da.subseq(start, width, other=db, from_other=from_b)
    with pytest.raises(SarlaccError, match="a second batch is selected but not given"):
        da.subseq([1] * len(a), [1] * len(a), other=None, from_other=from_b)


# ---- scramble -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCRAMBLE_COUNTS)
def test_scramble_equals_restatement_and_oracle(oracle, n):
    uploaded = {}
    for what, seqs, quals, seed, ws, wq in R.scramble_cases():
        if len(seqs) != n:
            continue
        if len(seqs[-1]) not in uploaded:
            uploaded[len(seqs[-1])] = _device_reads(seqs, quals)
        got = _download(uploaded[len(seqs[-1])].scramble(seed))
        _same(got, (ws, wq), what)
        _same(got, R.oracle_scramble(oracle, seqs, quals, seed), what + ", oracle")
        for r, (s, q, gs, gq) in enumerate(zip(seqs, quals, *got)):
            # the multiset is kept, and bases and qualities carry one permutation (quality p & 0xff names its
            # position up to 256; the longer reads are covered by the comparison above)
            assert sorted(gs) == sorted(s) and sorted(gq) == sorted(q), (what, r)
            if len(s) <= 256:
                assert gs == bytes(s[p] for p in gq), (what, r)


def test_scramble_of_a_read_depends_on_seed_index_and_length_only():
    rng = np.random.default_rng(9)
    shared = {3: R.read(rng, 1000), 64: R.read(rng, 64), 100: R.read(rng, 777)}
    outs = []
    for n, fill in ((101, 5), (130, 300)):
        seqs = [shared.get(r, R.read(rng, (r * 7 + fill) % 90)) for r in range(n)]
        quals = [R.quality(len(s)) for s in seqs]
        got = _download(_device_reads(seqs, quals).scramble(2 ** 63 + 12345))
        outs.append({r: (got[0][r], got[1][r]) for r in shared})
        want = R.scramble([shared[r] for r in shared], [R.quality(len(shared[r])) for r in shared], 0)   # (not the same index: differs)
        assert all(outs[-1][r][0] != w for r, w in zip(shared, want[0]))
    assert outs[0] == outs[1]
    for r, s in shared.items():
        perm = R.permutation(2 ** 63 + 12345, r, len(s))
        assert outs[0][r] == (bytes(s[p] for p in perm), bytes(p & 0xff for p in perm))


# ---- strand choice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s1,s2", R.STRAND_SECTIONS)
@pytest.mark.parametrize("n", R.STRAND_COUNTS)
def test_strand_choice_on_built_blocks(n, s1, s2):
    from sarlacc_amd import _lib, generics
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    raw = R.strand_blocks(n, s1, s2)
    sections = (s1, s2, s1, s2)
    dev = [(DevBuffer.from_numpy(b), n, s) for b, s in zip(raw, sections)]
    host = [R.block_tuple(b, n, s) for b, s in zip(raw, sections)]
    rows1, rows2, rev = DeviceReads.choose_strand(*dev)
    want1, want2, want_rev = R.choose_strand(*host)
    assert rev.tolist() == want_rev.tolist() == generics._resolve_strand(*(h[0] for h in host))[0].tolist()
    assert R.same_rows(rows1, want1) and R.same_rows(rows2, want2)
    # the blocks as they lie in HBM, the section row of a block without sections included: outputs that start as 0xEE
    out1, out2 = DevBuffer.from_numpy(np.full(raw[0].size, 0xEE, np.uint8)), DevBuffer.from_numpy(np.full(raw[1].size, 0xEE, np.uint8))
    d_rev = DevBuffer.from_numpy(np.full(n, 0xEE, np.uint8))
    _lib.check(_lib.lib().sarlacc_dev_choose_strand(dev[0][0], dev[1][0], dev[2][0], dev[3][0], n, s1, s2, out1, out2, d_rev, None))
    assert d_rev.to_numpy(np.uint8, n).tolist() == want_rev.astype(np.uint8).tolist()
    full = [R.block_tuple(b, n, s, hidden=True) for b, s in zip(raw, sections)]
    full1, full2, _ = R.choose_strand(*full)
    for out, want, s, size in ((out1, full1, s1, raw[0].size), (out2, full2, s2, raw[1].size)):
        got = R.block_tuple(out.to_numpy(np.uint8, size).copy(), n, s, hidden=True)
        assert R.same_rows(got, want), (n, s1, s2)


def test_strand_choice_refuses_blocks_of_different_shapes():
    from sarlacc_amd._lib import SarlaccError
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    raw = R.strand_blocks(4, 2, 1)
    cs, ce, rs, re = ((DevBuffer.from_numpy(b), 4, s) for b, s in zip(raw, (2, 1, 2, 1)))
    for blocks in ((cs, ce, (rs[0], 3, 2), re), (cs, (ce[0], 5, 1), rs, re), (cs, ce, (rs[0], 4, 1), re), (cs, ce, rs, (re[0], 4, 0))):
        with pytest.raises(SarlaccError, match="result blocks of different shapes"):
            DeviceReads.choose_strand(*blocks)


# ---- refusals on the host -----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_a_launch():
    from sarlacc_amd._lib import SarlaccError
    seqs, quals = R.batch((5, 0, 9, 3), 103)
    dev, other = _device_reads(seqs, quals), _device_reads(seqs[:3], quals[:3])
    for idx in ([-1], [0, 4], [2, -4, 1]):
        with pytest.raises(SarlaccError, match="'idx'"):
            dev.realize(idx, [0] * len(idx))
    for kw, name in (({"reversed_": [0]}, "reversed_"), ({"trim_start": [1, 1, 1]}, "trim_start"), ({"trim_end": [3]}, "trim_end")):
        args = dict(idx=[0, 2], reversed_=[0, 1], trim_start=[1, 1], trim_end=[3, 3])
        args.update(kw)
        with pytest.raises(SarlaccError, match="'%s'" % name):
            dev.realize(**args)
    for start, width, sel, name in (([1] * 3, [1] * 4, None, "start"), ([1] * 4, [1] * 5, None, "width"), ([1] * 4, [1] * 4, [0] * 3, "from_other")):
        with pytest.raises(SarlaccError, match="'%s'" % name):
            dev.subseq(start, width, other=dev if sel is not None else None, from_other=sel)
    with pytest.raises(SarlaccError, match="'other'"):
        dev.subseq([1] * 4, [0] * 4, other=other, from_other=[0] * 4)
    with pytest.raises(SarlaccError, match="'tolerance'"):
        dev.front_and_back(-1)


# ---- unmask -------------------------------------------------------------------------------------------------------
def _device_unmask(rows, origs):
    from sarlacc_amd import calls
    from sarlacc_amd._lib import SarlaccError
    try:
        return [s.encode() for s in calls.unmask_alignment(rows, origs)]
    except SarlaccError as e:
        return str(e)


def _oracle_unmask(oracle, rows, origs):
    try:
        return [s.encode() for s in oracle.unmask_alignment(rows, origs)]
    except oracle.OracleError as e:
        return str(e)


def test_unmask_at_every_width_and_refusal(oracle):
    served = refused = 0
    for what, rows, origs in R.unmask_cases():
        got = _device_unmask(rows, origs)
        want = R.unmask(rows, origs)
        assert got == want, (what, got if isinstance(got, str) or isinstance(want, str) else _differing(got, want))
        assert got == _oracle_unmask(oracle, rows, origs), what
        served += isinstance(got, list)
        refused += isinstance(got, str)
    assert served >= len(R.UNMASK_WIDTHS) and refused >= 9


def test_unmask_more_rows_than_the_grid_holds(oracle):
    nrows = 32 * _cus() + 37
    rows, origs = R.unmask_many(nrows)
    got = _device_unmask(rows, origs)
    want = R.unmask(rows, origs)
    assert isinstance(want, list) and got == want, _differing(got, want)
    assert got == _oracle_unmask(oracle, rows, origs)
    bad = 32 * _cus() + 20         # the only bad row is one the grid reaches in its second round
    rows, origs = R.unmask_many(nrows, bad)
    assert R.unmask(rows[:bad], origs[:bad]) == want[:bad] and R.unmask(rows, origs) == R.LENGTHS
    assert _device_unmask(rows, origs) == R.LENGTHS == _oracle_unmask(oracle, rows, origs)


# ---- mask ---------------------------------------------------------------------------------------------------------
def _masked(fn, error, *args):
    try:
        return fn(*args)
    except error as e:
        return str(e)


def test_mask_more_bases_than_the_grid_holds(oracle, oenc, enc):
    from sarlacc_amd import SarlaccError, calls
    grid = 16 * _cus() * 256
    total = grid + grid // 4
    seqs, quals = R.mask_batch(total)
    for thr in (0.01, 0.2):
        got = calls.mask_bad_bases(seqs, quals, enc, thr)
        want = oracle.mask_bad_bases(seqs, quals, oenc, thr)
        assert got == want, (thr, _differing(got, want))
        flat = "".join(got)
        assert 0 < flat.count("N") < total and flat[grid:].count("N") > 0
    # one quality below the encoding's lowest character where only the second round of the grid looks
    low, r = R.with_byte(quals, grid + grid // 8, 32)
    assert r > 0
    want = _masked(oracle.mask_bad_bases, oracle.OracleError, seqs, low, oenc, 0.2)
    assert want == "quality cannot be lower than smallest encoded value"
    assert _masked(calls.mask_bad_bases, SarlaccError, seqs, low, enc, 0.2) == want
    # a quality byte from 0x80 on is a negative character
    high, _ = R.with_byte(quals, grid // 2, 0x80)
    assert _masked(oracle.mask_bad_bases, oracle.OracleError, seqs, high, oenc, 0.2) == want
    assert _masked(calls.mask_bad_bases, SarlaccError, seqs, high, enc, 0.2) == want
    high, _ = R.with_byte(quals, grid + 5, 0xff)
    assert _masked(calls.mask_bad_bases, SarlaccError, seqs, high, enc, 0.2) == want


def test_mask_message_order(oracle, oenc, enc):
    from sarlacc_amd import SarlaccError, calls
    seqs, quals = R.mask_batch(3000, 12)
    short = list(quals)
    short[6] = short[6][:-1]                                      # the first length mismatch: read 7
    early, r_early = R.with_byte(short, sum(map(len, short[:2])) + 1, 32)
    late, r_late = R.with_byte(short, sum(map(len, short[:9])) + 1, 32)
    same, r_same = R.with_byte(short, sum(map(len, short[:6])), 32)
    assert (r_early, r_late, r_same) == (2, 9, 6)
    for what, q, message in (("low quality in an earlier read", early, "quality cannot be lower than smallest encoded value"),
                             ("low quality only in a later read", late, "sequence and quality strings should have the same length"),
                             ("low quality in the read of the mismatch", same, "sequence and quality strings should have the same length"),
                             ("no low quality", short, "sequence and quality strings should have the same length")):
        assert _masked(oracle.mask_bad_bases, oracle.OracleError, seqs, q, oenc, 0.1) == message, what
        assert _masked(calls.mask_bad_bases, SarlaccError, seqs, q, enc, 0.1) == message, what
