"""A family of quality encodings for the parity tests: every table here passes the reference's check (names consecutive
as signed chars, probabilities non-increasing), and each one moves something the kernels derive from the table -- its
length (LDS row strides, the clamp to the last entry, which vote kernel runs), its first name (the offset, negative for
names at or above byte 128) or its entries (the constants of adaptor_align's integer locator, -inf costs).

A table is given twice: as (errors, names) in the form the oracle takes, and as the package's Encoding.  Names are bytes;
quality strings drawn for a table are bytes too, since many of these names are not printable.
"""
import numpy as np

from sarlacc_amd.encoding import Encoding, illumina_encoding, phred_encoding, solexa_encoding


def _names(first, n):
    """n consecutive names from byte `first`, continuing through byte 255 into 0, 1, ... (consecutive as signed chars as
    long as the run does not pass from byte 127 to byte 128)."""
    return bytes((first + k) & 0xFF for k in range(n))


def _signed(b):
    return b - 256 if b >= 128 else b


class Table:
    """name; enc (sarlacc_amd.encoding.Encoding); oenc ((errors, names) for the oracle)."""

    def __init__(self, name, errors, names):
        self.name = name
        self.errors = np.ascontiguousarray(errors, dtype=np.float64)
        self.names = bytes(names)
        self.enc = Encoding(self.errors, self.names)
        self.oenc = (self.errors, self.names)

    def __repr__(self):
        return self.name

    def __len__(self):
        return len(self.names)

    @property
    def first(self):
        """The first name as the reference reads it: a signed char."""
        return _signed(self.names[0])

    def pool(self, past=6):
        """Every quality byte the table accepts and these tests draw: the first name, every entry, the last entry, and up
        to `past` characters beyond it (they clamp to the last entry), as far as signed chars go (127)."""
        top = min(127, self.first + len(self) - 1 + past)
        return np.array([v & 0xFF for v in range(self.first, top + 1)], dtype=np.uint8)

    def below(self):
        """A quality byte below the first name (the reference's error), or None when the table starts at -128."""
        return None if self.first == -128 else bytes([(self.first - 1) & 0xFF])

    def shifted(self):
        """The same names on the table moved by one entry: every character gets its neighbour's probability (a wrong
        table for the comparisons to notice)."""
        return self.errors[1:].copy(), self.names[:-1]

    def cut(self):
        """The table without its last entry (wrong for the last name and everything beyond it)."""
        return self.errors[:-1].copy(), self.names[:-1]


def draw_quals(table, lengths, seed, lo=None, hi=None):
    """One quality string (bytes) per length.  Characters come from table.pool(); the first len(pool) characters of the
    batch run through the whole pool once, so a batch at least that long holds the first name, every entry, the last entry
    and the characters past it.  lo / hi restrict the draw to table indices lo..hi (hi may exceed the last index)."""
    rng = np.random.default_rng(seed)
    pool = table.pool()
    if lo is not None or hi is not None:
        pool = pool[(0 if lo is None else lo):(len(pool) if hi is None else hi + 1)]
    lengths = [int(x) for x in lengths]
    total = sum(lengths)
    flat = pool[rng.integers(0, len(pool), total)]
    if total >= len(pool):
        flat[:len(pool)] = rng.permutation(pool)
    out, at = [], 0
    for n in lengths:
        out.append(flat[at:at + n].tobytes())
        at += n
    return out


def _decades(n, per_decade):
    return np.power(10.0, -np.arange(n, dtype=np.float64) / per_decade)


def _package(name, enc):
    return Table(name, enc.errors, enc.names)


TABLES = [
    _package("phred", phred_encoding()),                                      # the control: 94 entries from '!'
    _package("illumina", illumina_encoding()),
    _package("solexa", solexa_encoding()),
    Table("one", [0.05], b"I"),
    Table("two", [0.3, 0.001], b"56"),
    Table("n127_from_1", _decades(127, 12.0), _names(1, 127)),                # the largest table k_consensus_qf accepts
    Table("n128_high", _decades(128, 13.0), _names(128, 128)),                # bytes 128..255: the offset is -128
    Table("n60_high", _decades(60, 6.0), _names(160, 60)),                    # short enough for k_consensus_qf, negative offset
    Table("n149_wrap", _decades(149, 15.0), _names(200, 149)),                # the largest table k_consensus_code accepts
    Table("n150_wrap", _decades(150, 15.0), _names(200, 150)),                # ... and one past it; names run through 255 into 0, 1, ...
    Table("n256", _decades(256, 26.0), _names(128, 256)),                     # every byte is a name: run_align's limit
    Table("tiny", np.power(10.0, np.linspace(-0.3, -30.0, 120)), _names(8, 120)),   # large finite mismatch costs: the locator's k drops
    Table("zero_tail", np.concatenate([np.power(10.0, np.linspace(-0.5, -8.0, 40)), [1e-300, 0.0]]), _names(48, 42)),   # mismatch cost -inf
    Table("one_head", [1.0, 0.5, 0.1, 0.01, 1e-3, 1e-4], _names(65, 6)),      # match cost -inf at the first name
    Table("ties", np.full(30, 0.75), _names(35, 30)),                         # "should decrease" admits equal entries
]
BY_NAME = {t.name: t for t in TABLES}
TABLE_IDS = [t.name for t in TABLES]

# Tables the reference's check refuses, with its message.  257 names cannot be consecutive as signed chars: wherever the run
# starts it passes from byte 127 to byte 128.
REJECTED = [
    ("empty", np.zeros(0), b"", "encoding vector must be non-empty and named"),
    ("not_consecutive", np.array([0.5, 0.1, 0.01]), b"ABD", "names of encoding vector should increase consecutively"),
    ("past_127", _decades(10, 10.0), _names(123, 10), "names of encoding vector should increase consecutively"),
    ("increasing", np.array([0.5, 0.1, 0.2]), b"ABC", "error probabilities should decrease"),
    ("n257", _decades(257, 26.0), _names(128, 257), "names of encoding vector should increase consecutively"),
]
