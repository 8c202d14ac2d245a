"""A plain-Python rANS coder on Python integers: the yardstick of test_rans_host.py and test_rans_gpu.py.   *** TEST INFRASTRUCTURE ***

Written from the format's definition (the header comment of csrc/rans.hip, and CompressAI's BufferedRansEncoder / RansDecoder over ryg's rans64.h); it calls neither the
library nor oracle/rans_oracle.c, and no value in it has a fixed width:

  * rANS64, lower bound L = 2^31, 16-bit probabilities.  Coding (start, freq): while x >= (L >> 16 << 32) * freq a 32-bit word leaves the state, then
    x = (x // freq << 16) + x % freq + start.  Four raw bits v: the same with freq = 2^12 and x = x << 4 | v.  Words are emitted BACK TO FRONT and the final state
    goes in front of them, low word first, so the decoder reads the stream forwards.
  * A symbol s on row r: value = s - offset[r]; values 0 .. size[r] - 3 are coded with their own (start, freq); everything else is the row's LAST symbol (size - 2, the
    escape) followed by raw = -2 value - 1 (value < 0) or 2 (value - (size - 2)) as: the number of 4-bit nibbles in base 15 (digits of 15 while more than 14 remain, then
    the rest), then the nibbles, low to high.
  * The encoder pushes these operations in reading order and codes them in REVERSE; the decoder pops them in reading order.

Why not the C oracle alone: oracle/rans_oracle.c restates CompressAI's `while ((raw_val >> (n_bypass * 4)) != 0)` on a 32-bit value, which shifts by 32 for
raw >= 2^28 and never returns, and a row of size 2 (frequency 2^16) ends it in SIGFPE.  It is valid for raw < 2^28 and rows of 3 entries or more only, so the library's
8-nibble escapes have no reference but this file.  test_rans_host.py pins this coder to the C oracle byte for byte wherever the oracle is valid.
"""
import struct

import numpy as np
import torch

L = 1 << 31
PREC = 16
NIBBLE = 4
MAX_DIGIT = 15
MAGIC = b"RCR1"


class Rows:
    """Tables as Python lists: rows[r] = the row's `size` cumulative frequencies, offs[r] = its offset."""

    def __init__(self, tables):
        cdf = np.asarray(tables["_quantized_cdf"]).astype(np.int64)
        sizes = np.asarray(tables["_cdf_length"]).reshape(-1).astype(np.int64)
        self.rows = [cdf[r, :int(sizes[r])].tolist() for r in range(cdf.shape[0])]
        self.offs = [int(o) for o in np.asarray(tables["_offset"]).reshape(-1)]
        for r, row in enumerate(self.rows):
            assert len(row) >= 3 and row[0] == 0 and row[-1] == 1 << PREC and all(b > a for a, b in zip(row, row[1:])), f"row {r} is not a quantised CDF with an escape"


def _rows(tables):
    return tables if isinstance(tables, Rows) else Rows(tables)


def _ints(a):
    return [int(v) for v in (a.reshape(-1).tolist() if hasattr(a, "reshape") else a)]


def split(symbol, row, offset):
    """-> (value coded with the row's frequencies, raw or None)."""
    escape = len(row) - 2
    value = symbol - offset
    if value < 0:
        return escape, -2 * value - 1
    if value >= escape:
        return escape, 2 * (value - escape)
    return value, None


def nibbles(raw):
    n = 0
    while raw >> (NIBBLE * n):
        n += 1
    return n


def encode(symbols, indexes, tables, max_nibbles=8):
    """One stream.  An escape longer than max_nibbles is refused; max_nibbles = 9 lets a symbol past the 32-bit range (raw >= 2^32) through, as a well-formed stream that
    no decoder of the format may accept."""
    t = _rows(tables)
    ops = []                                              # reading order: (start, freq) or (nibble,)
    for s, r in zip(_ints(symbols), _ints(indexes)):
        if not 0 <= r < len(t.rows):
            raise IndexError(f"CDF index {r} out of range")
        row = t.rows[r]
        value, raw = split(s, row, t.offs[r])
        ops.append((row[value], row[value + 1] - row[value]))
        if raw is not None:
            n = nibbles(raw)
            if n > max_nibbles:
                raise ValueError(f"escape of {n} nibbles")
            left = n
            while left >= MAX_DIGIT:
                ops.append((MAX_DIGIT,))
                left -= MAX_DIGIT
            ops.append((left,))
            ops.extend(((raw >> (NIBBLE * j)) & 15,) for j in range(n))
    x, words = L, []
    for op in reversed(ops):
        if len(op) == 2:
            start, freq = op
            if x >= ((L >> PREC) << 32) * freq:
                words.append(x & 0xFFFFFFFF)
                x >>= 32
            x = ((x // freq) << PREC) + x % freq + start
        else:
            if x >= ((L >> PREC) << 32) << (PREC - NIBBLE):
                words.append(x & 0xFFFFFFFF)
                x >>= 32
            x = (x << NIBBLE) | op[0]
    words.append(x >> 32)
    words.append(x & 0xFFFFFFFF)
    words.reverse()
    return struct.pack(f"<{len(words)}I", *words)


def decode(stream, indexes, tables):
    """The symbols of one stream.  ValueError on a read past the stream's end and on an escape of more than 8 nibbles."""
    t = _rows(tables)
    if len(stream) < 8 or len(stream) % 4:
        raise ValueError("a stream is whole 32-bit words, at least the flushed state")
    words = struct.unpack(f"<{len(stream) // 4}I", stream)
    x, pos = words[0] | (words[1] << 32), 2

    def renorm():
        nonlocal x, pos
        if x < L:
            if pos >= len(words):
                raise ValueError("read past the end of the stream")
            x = (x << 32) | words[pos]
            pos += 1

    def bits():
        nonlocal x
        v = x & 15
        x >>= NIBBLE
        renorm()
        return v

    out = []
    for r in _ints(indexes):
        if not 0 <= r < len(t.rows):
            raise IndexError(f"CDF index {r} out of range")
        row = t.rows[r]
        cum = x & 0xFFFF
        value = _search(row, cum)
        x = (row[value + 1] - row[value]) * (x >> PREC) + cum - row[value]
        renorm()
        if value == len(row) - 2:
            digit = bits()
            n = digit
            while digit == MAX_DIGIT:
                if n > 8:
                    break
                digit = bits()
                n += digit
            if n > 8:
                raise ValueError(f"escape of {n} nibbles")
            raw = 0
            for j in range(n):
                raw |= bits() << (NIBBLE * j)
            value = -(raw + 1) // 2 if raw & 1 else raw // 2 + value
        out.append(value + t.offs[r])
    return np.asarray(out, dtype=np.int64)


def _search(row, cum):
    lo, hi = 0, len(row) - 1                                # the last j with row[j] <= cum
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if row[mid] <= cum:
            lo = mid
        else:
            hi = mid
    return lo


# ---- conditions on an input ---------------------------------------------------------------------------------------------------------------------------------------------
def escape_classes(symbols, indexes, tables):
    """{(nibbles, sign): count} over the escaped symbols; sign is -1 for value < 0 and +1 otherwise (the 0-nibble escape, value == size - 2, has sign +1 only)."""
    t = _rows(tables)
    out = {}
    for s, r in zip(_ints(symbols), _ints(indexes)):
        raw = split(s, t.rows[r], t.offs[r])[1]
        if raw is not None:
            k = (nibbles(raw), -1 if raw & 1 else 1)
            out[k] = out.get(k, 0) + 1
    return out


def support_pairs(symbols, indexes, tables):
    """The (row, value) pairs that are coded with a frequency of their own."""
    t = _rows(tables)
    out = set()
    for s, r in zip(_ints(symbols), _ints(indexes)):
        value, raw = split(s, t.rows[r], t.offs[r])
        if raw is None:
            out.add((r, value))
    return out


def all_classes(seven_max=False):
    top = 7 if seven_max else 8
    return [(0, 1)] + [(n, sign) for n in range(1, top + 1) for sign in (1, -1)]


def all_pairs(tables, first_row=0):
    t = _rows(tables)
    return {(r, v) for r in range(first_row, len(t.rows)) for v in range(len(t.rows[r]) - 2)}


def assert_covered(symbols, indexes, tables, first_row=0, seven_max=False, least=20):
    """The two conditions every test puts on its edge symbols before it uses them: each escape class at least `least` times (17 classes, 15 with seven_max) and every
    (row, in-support symbol) pair of the rows from first_row on.  Conditions on the input, checked on the CPU; nothing here is measured."""
    got = escape_classes(symbols, indexes, tables)
    want = all_classes(seven_max)
    assert set(got) == set(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    assert min(got.values()) >= least, sorted(got.items())
    missing = all_pairs(tables, first_row) - support_pairs(symbols, indexes, tables)
    assert not missing, sorted(missing)[:10]


# ---- the edge inputs ----------------------------------------------------------------------------------------------------------------------------------------------------
def edge_tables():
    """Six rows with frequency 1 at both ends of a row and as the escape symbol, and 65535, 2^15 and 2^12: the edges of the division-free state update's reciprocal."""
    rows = [[0, 65535, 65536],                                                                    # A: escape of frequency 1
            [0, 1, 65536],                                                                        # B: escape of frequency 65535
            [0, 32768, 65536],                                                                    # C
            [0, 1, 2, 3, 65535, 65536],                                                           # D
            [0, 4096, 4097, 36865, 36866, 65536],                                                 # E
            np.concatenate([[0], np.cumsum([1] * 200 + [65536 - 300] + [1] * 99 + [1])]).tolist()]   # F: 300 symbols below the escape
    offsets = [0, -1, 3, -2, 0, -150]
    assert len(rows[5]) == 302 and rows[5][-1] == 65536
    cdf = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int32)
    for i, r in enumerate(rows):
        cdf[i, :len(r)] = r
    return {"_quantized_cdf": torch.from_numpy(cdf), "_cdf_length": torch.tensor([len(r) for r in rows], dtype=torch.int32),
            "_offset": torch.tensor(offsets, dtype=torch.int32)}


def append_tables(t, extra):
    """The rows of `extra` behind the rows of `t`, zero-padded to one width."""
    a, b = t["_quantized_cdf"].int(), extra["_quantized_cdf"].int()
    cdf = torch.zeros(a.shape[0] + b.shape[0], max(a.shape[1], b.shape[1]), dtype=torch.int32)
    cdf[:a.shape[0], :a.shape[1]] = a
    cdf[a.shape[0]:, :b.shape[1]] = b
    cat = lambda k: torch.cat([t[k].int().reshape(-1), extra[k].int().reshape(-1)])
    return {"_quantized_cdf": cdf, "_cdf_length": cat("_cdf_length"), "_offset": cat("_offset")}


def edge_symbols(n, seed, seven_max=False, tables=None, first_row=0):
    """(symbols, indexes) int32 on the rows of edge_tables() (or the rows of `tables` from first_row on): a body uniform over each row's in-support symbols, every
    (row, symbol) pair planted once, and max(n // 8, 360) planted escapes that walk the classes in turn (nibble counts 0..8, or 0..7 with seven_max, both signs), the
    first two of a class at the class's smallest and largest raw value, |symbol - offset| <= 2^30.  Positions are a seeded permutation; an n too small for all of
    it gets a prefix of the escapes, and assert_covered says so."""
    t = _rows(tables if tables is not None else edge_tables())
    rng = np.random.default_rng(seed)
    idx = rng.integers(first_row, len(t.rows), n)
    support = np.asarray([len(row) - 2 for row in t.rows], dtype=np.int64)
    sym = np.floor(rng.random(n) * support[idx]).astype(np.int64) + np.asarray(t.offs, dtype=np.int64)[idx]
    where = rng.permutation(n).tolist()
    classes = all_classes(seven_max)
    seen = {}
    for k in range(min(max(n // 8, 360), n)):
        i = where.pop()
        nb, sign = classes[k % len(classes)]
        r = int(idx[i])
        escape = len(t.rows[r]) - 2
        if nb == 0:
            value = escape
        else:
            odd = 1 if sign < 0 else 0
            lo = 1 << (NIBBLE * (nb - 1))
            hi = min((1 << (NIBBLE * nb)) - 1, (1 << 31) - 1 if odd else (1 << 31) - 2 * escape)
            lo += (lo & 1) != odd
            hi -= (hi & 1) != odd
            rep = seen.get((nb, sign), 0)
            seen[(nb, sign)] = rep + 1
            raw = lo if rep == 0 else hi if rep == 1 else (int(rng.integers(lo, hi + 1)) & ~1) | odd
            raw = min(max(raw, lo), hi)
            value = -(raw + 1) // 2 if odd else raw // 2 + escape
        assert abs(value) <= 1 << 30
        sym[i] = value + t.offs[r]
    pairs = sorted(all_pairs(t, first_row))
    for r, v in pairs[:len(where)]:
        i = where.pop()
        idx[i] = r
        sym[i] = v + t.offs[r]
    return sym.astype(np.int32), idx.astype(np.int32)


def worst_case(m):
    """m symbols on row A of edge_tables(), each -2^30: an 8-nibble escape through an escape symbol of frequency 1, 16 + 4 + 32 = 52 bits a symbol, the most the
    format can spend on a 32-bit symbol."""
    return np.full(m, -(1 << 30), dtype=np.int32), np.zeros(m, dtype=np.int32)


# ---- the "chunked" container -------------------------------------------------------------------------------------------------------------------------------------------
def split_container(blob):
    """-> (n, chunk, [the chunk streams]); the header's arithmetic is asserted."""
    magic, n, chunk, n_chunks = struct.unpack_from("<4sIII", blob, 0)
    assert magic == MAGIC and chunk >= 1 and n_chunks == -(-n // chunk), (magic, n, chunk, n_chunks)
    sizes = struct.unpack_from(f"<{n_chunks}I", blob, 16)
    p, out = 16 + 4 * n_chunks, []
    for s in sizes:
        out.append(blob[p:p + s])
        p += s
    assert p == len(blob), (p, len(blob))
    return n, chunk, out


def container(n, chunk, streams):
    assert len(streams) == -(-n // chunk)
    return struct.pack("<4sIII", MAGIC, n, chunk, len(streams)) + struct.pack(f"<{len(streams)}I", *(len(s) for s in streams)) + b"".join(streams)


# ---- the inputs of test_rans_gpu.py (test_rans_host.py asserts the two conditions on every one of them) ---------------------------------------------------------------
ENC_CHUNKS = (1, 3, 15, 16, 17, 31, 33, 250, 2048)          # the edges of the serial kernel's batches of 16 and of the decoder's look-ahead of 8; 250 = 2 mod 4
ENC_COUNTS = (1, 63, 64, 65, 129)                           # chunk counts: the serial kernel's blocks of 64 lanes filled and crossed, an odd stride of the operation layout


def encoder_cases(chunk):
    """The n of every encoder call with this chunk length: each chunk count with a last chunk of 1 symbol, of chunk - 1 symbols and a full one (all three for the
    short chunks, in turn at 250; 2048 takes one chunk three ways and 65 chunks), and one further call that brings the symbols of the list to 1500, enough for the two
    conditions."""
    lasts = sorted({1, chunk - 1, chunk} - {0})
    if chunk == 2048:
        ns = [1, 2047, 2048, 64 * 2048 + 1]
    elif chunk == 250:
        ns = [(c - 1) * chunk + lasts[i % 3] for i, c in enumerate(ENC_COUNTS)]
    else:
        ns = [(c - 1) * chunk + last for c in ENC_COUNTS for last in lasts]
    if sum(ns) < 1500:
        ns.append(1500 - sum(ns))
    return ns


def sliced(ns, seed, **kw):
    """edge_symbols(sum(ns)) cut into consecutive calls of ns symbols: -> (symbols, indexes, [(start, n)])."""
    sym, idx = edge_symbols(sum(ns), seed, **kw)
    starts = np.concatenate([[0], np.cumsum(ns)[:-1]]).tolist()
    return sym, idx, list(zip(starts, ns))


ONE_CHUNK_NS = (1, 17, 3000)                                                                   # chunk == n
DEC_CASES = ((1, 130), (3, 212), (7, 216), (8, 241), (9, 278), (16, 805), (17, 851), (31, 1270), (250, 2499), (2048, 4103))   # (chunk, n): 0, 1, 2 and 3 mod 4
LANE_CHUNKS = (3, 4)
ARENA_CHUNKS = (1, 16, 17, 512)
SEEDS = {"encoder": 100, "one_chunk": 200, "decoder": 300, "lanes": 400, "errors": 500, "second_run": 600, "grid_cap": 700}


def lanes_for(n_chunks, cu):
    """The LDS decoder's chunks per wave (rc_rans_decode_chunks): as few as give every CU two blocks, 64 at the most."""
    return min(64, max(1, -(-n_chunks // (2 * cu))))


def lane_cases(cu):
    """(lanes, n_chunks): the smallest chunk counts that give 2 and 3 chunks per wave, and the smallest that gives 64."""
    return [(2, 2 * cu + 1), (3, 4 * cu + 1), (64, 63 * 2 * cu + 1)]
