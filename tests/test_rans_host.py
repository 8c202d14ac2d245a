"""No GPU: the plain-Python coder of tests/rans_ref.py against the C oracle where the oracle is valid, the library's host coder against the Python coder everywhere, the
conditions on every input of test_rans_gpu.py, the scratch bound of rc_rans_chunk_words, and the coverage table of test_rans_gpu.py against the header."""
import os
import re

import numpy as np
import pytest
import torch

import codec_ref as C
import entropy_oracle as E
import rans_ref as R
from realcamnet_amd import _lib, bitstream
from test_bitstream import _symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITSTREAM_CASES = ((1, 1), (4097, 2), (70001, 3), (3000, 4))           # test_bitstream.py's (n, seed)


def lib_tables(t, device="cpu"):
    return bitstream.Tables(t["_quantized_cdf"], t["_cdf_length"], t["_offset"], device)


def gaussian():
    return E.gc_update(E.get_scale_table())


def oracle_inputs():
    """(what, tables, symbols, indexes) the C oracle can take: the Gaussian rows with test_bitstream.py's symbols, the edge rows with escapes of at most 7 nibbles."""
    g = gaussian()
    for n, seed in BITSTREAM_CASES:
        yield (f"gaussian n {n}", g) + _symbols(n, g, seed)
    e = R.edge_tables()
    sym, idx = R.edge_symbols(4000, 7, seven_max=True)
    R.assert_covered(sym, idx, e, seven_max=True)
    yield ("edge rows, 7 nibbles at most", e, sym, idx)


def python_only_inputs():
    e = R.edge_tables()
    sym, idx = R.edge_symbols(4000, 8)
    R.assert_covered(sym, idx, e)
    yield ("edge rows", e, sym, idx)
    yield ("worst case", e) + R.worst_case(512)


def test_reference_equals_the_c_oracle():
    """rans_ref.encode is entropy_oracle.encode_with_indexes byte for byte and the two decoders return the symbols.  The C oracle is never given raw >= 2^28 or a row of
    size 2: it restates CompressAI's `while ((raw_val >> (n_bypass * 4)) != 0)` on a 32-bit value, which for raw >= 2^28 shifts by 32 and does not return, and a row of
    size 2 has the single frequency 2^16, which it divides by as a 16-bit zero (SIGFPE).  Both preconditions are asserted here on every input it gets."""
    for what, t, sym, idx in oracle_inputs():
        assert int(np.asarray(t["_cdf_length"]).min()) >= 3, what
        assert max(k[0] for k in R.escape_classes(sym, idx, t) or {(0, 1)}) <= 7, what
        rows = R.Rows(t)
        want = E.encode_with_indexes(sym, idx, t)
        assert R.encode(sym, idx, rows) == want, what
        assert np.array_equal(R.decode(want, idx, rows), sym), what
        assert np.array_equal(E.Decoder(want).decode_stream(idx, t), sym), what


def test_host_coder_equals_the_reference():
    """bitstream.encode(fmt="compressai") is the reference's stream and Decoder(fmt="compressai") returns the symbols with its state carried over a split, on the oracle's
    inputs and on the two only the Python coder can take: the full edge symbols (8-nibble escapes) and worst_case(512)."""
    for what, t, sym, idx in list(oracle_inputs()) + list(python_only_inputs()):
        tables = lib_tables(t)
        want = R.encode(sym, idx, t)
        assert bitstream.encode(torch.from_numpy(sym), torch.from_numpy(idx), tables, "compressai") == want, what
        dec = bitstream.Decoder(want, tables, "cpu", "compressai")
        cut = len(sym) // 3
        got = torch.cat([dec.decode(torch.from_numpy(idx[:cut])), dec.decode(torch.from_numpy(idx[cut:]))]).numpy()
        assert np.array_equal(got, sym), what
        assert np.array_equal(R.decode(want, idx, t), sym), what


def test_reference_decoder_refuses_what_the_format_forbids():
    e = R.edge_tables()
    sym, idx = R.edge_symbols(700, 3)
    stream = R.encode(sym, idx, e)
    for bad in (stream[:-4], stream[:8], stream[:len(stream) // 8 * 4]):
        with pytest.raises(ValueError, match="past the end"):
            R.decode(bad, idx, e)
    with pytest.raises(ValueError, match="escape of 9 nibbles"):
        R.encode([(1 << 31) + 400], [0], e)
    with pytest.raises(ValueError, match="escape of 9 nibbles"):
        R.decode(R.encode([(1 << 31) + 400], [0], e, max_nibbles=9), [0], e)
    with pytest.raises(IndexError):
        R.encode([0], [6], e)
    with pytest.raises(IndexError):
        R.decode(stream, [-1], e)


def test_escape_classes_of_the_earlier_inputs():
    """What test_bitstream.py's symbols reach over its four sizes: five classes, none of 0, 1, 2, 6 or 8 nibbles (2^27 gives raw < 2^28: 7 nibbles, not 8)."""
    g = gaussian()
    rows, total = R.Rows(g), {}
    for n, seed in BITSTREAM_CASES:
        for k, v in R.escape_classes(*_symbols(n, g, seed), rows).items():
            total[k] = total.get(k, 0) + v
    assert total == {(3, 1): 64, (4, 1): 726, (5, -1): 367, (7, 1): 78, (7, -1): 78}, sorted(total.items())
    freq = np.diff(g["_quantized_cdf"].numpy().astype(np.int64), axis=1)
    assert int(freq.max()) == 65533 and int(g["_cdf_length"].min()) >= 5


def test_edge_tables_carry_the_edge_frequencies():
    rows = R.Rows(R.edge_tables())
    freqs = [[b - a for a, b in zip(row, row[1:])] for row in rows.rows]
    assert [len(r) for r in rows.rows] == [3, 3, 3, 6, 6, 302] and rows.offs == [0, -1, 3, -2, 0, -150]
    assert freqs[0] == [65535, 1] and freqs[1] == [1, 65535] and freqs[2] == [32768, 32768] and freqs[3] == [1, 1, 1, 65532, 1]
    assert freqs[4] == [4096, 1, 32768, 1, 28670]
    assert freqs[5] == [1] * 200 + [65236] + [1] * 99 + [1]
    assert all(sum(f) == 65536 for f in freqs)


def gpu_file_inputs():
    """Every input of test_rans_gpu.py (at 256 CUs), as (what, symbols, indexes, tables, first_row)."""
    e = R.edge_tables()
    for chunk in R.ENC_CHUNKS:
        sym, idx, _ = R.sliced(R.encoder_cases(chunk), R.SEEDS["encoder"] + chunk)
        yield f"encoder chunk {chunk}", sym, idx, e, 0
    sym, idx, _ = R.sliced(R.ONE_CHUNK_NS, R.SEEDS["one_chunk"])
    yield "one chunk", sym, idx, e, 0
    g = gaussian()
    for rows, entries in ((0, 0), (40, 1000)):
        t = R.append_tables(C.big_tables(g, rows, entries) if rows else g, e)
        sym, idx, _ = R.sliced([n for _, n in R.DEC_CASES], R.SEEDS["decoder"], tables=t, first_row=64 + rows)
        yield f"decoder, {64 + rows} rows in front", sym, idx, t, 64 + rows
    for chunk in R.LANE_CHUNKS:
        for lanes, n_chunks in R.lane_cases(256):
            sym, idx = R.edge_symbols((n_chunks - 1) * chunk + 1, R.SEEDS["lanes"] + 100 * chunk + lanes)
            yield f"lanes {lanes} chunk {chunk}", sym, idx, e, 0
    yield ("errors", *R.edge_symbols(2000, R.SEEDS["errors"]), e, 0)
    yield ("second run", *R.edge_symbols(5000, R.SEEDS["second_run"]), e, 0)
    yield ("past the grid cap (the repeated part)", *R.edge_symbols(4999, R.SEEDS["grid_cap"]), e, 0)


def test_inputs_of_the_gpu_file_meet_their_conditions():
    """All 17 escape classes (0 to 8 nibbles, both signs) at least 20 times and every (row, in-support symbol) pair, in every input the GPU file codes; the same
    assertion stands in front of every GPU test.  The encoder's call lists hold the chunk counts and last-chunk lengths the kernels' edges need."""
    for what, sym, idx, t, first_row in gpu_file_inputs():
        R.assert_covered(sym, idx, t, first_row=first_row)
        assert int(np.abs(sym.astype(np.int64) - np.asarray(t["_offset"]).astype(np.int64)[idx]).max()) == 1 << 30, what
    counts, lasts = set(), set()
    for chunk in R.ENC_CHUNKS:
        for n in R.encoder_cases(chunk):
            counts.add(-(-n // chunk))
            lasts.add((chunk, n - (-(-n // chunk) - 1) * chunk))
    assert set(R.ENC_COUNTS) <= counts
    assert all({(c, 1), (c, c), (c, max(c - 1, 1))} <= lasts for c in R.ENC_CHUNKS)
    assert {c % 4 for c, _ in R.DEC_CASES} == {0, 1, 2, 3}
    assert [R.lanes_for(n, 256) for _, n in R.lane_cases(256)] == [2, 3, 64] and [n for _, n in R.lane_cases(256)] == [513, 1025, 32257]
    assert [R.lanes_for(n - 1, 256) for _, n in R.lane_cases(256)] == [1, 2, 63]


@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 512, 2048])
def test_worst_case_stays_inside_the_scratch_bound(m):
    """rc_rans_chunk_words(m) = 2 m + 8 words can hold m symbols of 52 bits each, the most the format spends on a 32-bit symbol (16 for an escape symbol of frequency 1,
    4 for the length, 32 of nibbles), plus the flushed state."""
    e = R.edge_tables()
    sym, idx = R.worst_case(m)
    assert R.escape_classes(sym, idx, e) == {(8, -1): m}
    words = len(R.encode(sym, idx, e)) // 4
    cap = _lib.load().rc_rans_chunk_words(m)
    assert cap == 2 * m + 8 and words <= cap, (m, words, cap)
    assert words >= (52 * m + 31) // 32 + 1, (m, words)
    if m == 512:
        assert words == 834


def test_host_decoder_refuses_a_nine_nibble_escape():
    """A well-formed stream with one escape of 9 nibbles (a symbol past the 32-bit range): "truncated or corrupt", at the first symbol, in the middle, at the last."""
    e = R.edge_tables()
    tables = lib_tables(e)
    sym, idx = R.edge_symbols(700, 11)
    for at in (0, 350, 699):
        long = [int(s) for s in sym]
        long[at] = (1 << 31) + 400
        stream = R.encode(long, idx, e, max_nibbles=9)
        with pytest.raises(_lib.HipError, match="truncated or corrupt"):
            bitstream.Decoder(stream, tables, "cpu", "compressai").decode(torch.from_numpy(idx))
        got = bitstream.Decoder(R.encode(sym, idx, e), tables, "cpu", "compressai").decode(torch.from_numpy(idx))
        assert np.array_equal(got.numpy(), sym)


def test_tables_refuse_a_row_without_a_symbol_or_wider_than_the_table():
    """A row of size 2 is the escape alone with frequency 2^16: the device packs the frequency into 16 bits and would code it as 0 while the host codes 65536."""
    e = R.edge_tables()
    cdf, sizes, offs = e["_quantized_cdf"], e["_cdf_length"], e["_offset"]
    lib_tables(e)
    for row, size in ((0, 2), (3, 1), (5, 0), (1, 303), (2, -1)):
        bad = sizes.clone()
        bad[row] = size
        with pytest.raises(ValueError, match=f"row {row} "):
            bitstream.Tables(cdf, bad, offs, "cpu")
    one = torch.tensor([[0, 65536, 0]], dtype=torch.int32)
    with pytest.raises(ValueError, match="row 0 "):
        bitstream.Tables(one, torch.tensor([2], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), "cpu")


# ---- the coverage table of the GPU file -----------------------------------------------------------------------------------------------------------------------------
RANS_ENTRY_POINTS = {"rc_rans_chunk_words", "rc_rans_encode_scratch_bytes", "rc_rans_encode_chunks", "rc_rans_compact", "rc_rans_decode_chunks", "rc_rans_encode_host",
                     "rc_rans_decode_host"}
# how a test body reaches an entry point other than by the library handle (hip.rc_...)
REACHED_THROUGH = {"rc_rans_encode_chunks": r'encode_chunked\(', "rc_rans_compact": r'encode_chunked\(', "rc_rans_decode_chunks": r'decode_chunked\(',
                   "rc_rans_encode_host": r'bitstream\.encode\([^\n]*"compressai"\)', "rc_rans_decode_host": r'bitstream\.Decoder\([^\n]*"compressai"\)'}


def test_every_rans_entry_point_is_in_the_gpu_files_coverage_table():
    """Every rc_rans_* entry point of the header has a row in the docstring of test_rans_gpu.py and the other way round; the test a row names exists and its body reaches
    the entry point, by the library handle or through bitstream (encode_chunked / decode_chunked are the file's one-line wrappers of bitstream.encode / Decoder)."""
    header = open(os.path.join(ROOT, "include", "realcam_hip.h")).read()
    declared = set(re.findall(r"\b(rc_rans_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == RANS_ENTRY_POINTS, sorted(declared ^ RANS_ENTRY_POINTS)
    gpu = open(os.path.join(ROOT, "tests", "test_rans_gpu.py")).read()
    doc = gpu.split('"""')[1]
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(rc_[a-z0-9_]+)\s+(test_[a-z0-9_]+)", doc, flags=re.M)}
    assert set(rows) == RANS_ENTRY_POINTS, sorted(set(rows) ^ RANS_ENTRY_POINTS)
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^def (test_[a-z0-9_]+)\(.*?\n(.*?)(?=^\S|\Z)", gpu, flags=re.M | re.S)}
    assert "def encode_chunked(" in gpu and "def decode_chunked(" in gpu
    for entry, test in rows.items():
        assert test in bodies, (entry, test)
        how = [rf"\bhip\.{entry}\("] + ([REACHED_THROUGH[entry]] if entry in REACHED_THROUGH else [])
        assert any(re.search(p, bodies[test]) for p in how), (entry, test)
