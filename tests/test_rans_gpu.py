"""GPU: the entropy coder of csrc/rans.hip, chunk by chunk, against the plain-Python coder of tests/rans_ref.py.

Integer work: every assertion is an equality of bytes or of symbols.  The inputs are the edge rows of rans_ref.edge_tables() (frequencies 1, 2^12, 2^15, 65535, frequency 1
as the escape symbol) with rans_ref.edge_symbols(): a uniform body and planted escapes of every nibble count 0..8 and both signs.  Every test first asserts, through
rans_ref.assert_covered, that its input holds all 17 escape classes at least 20 times and every (row, in-support symbol) pair; test_rans_host.py asserts the same for all
of them without a GPU.

Coverage (entry point, the test that runs it; test_rans_host.py checks this table against the header):

    rc_rans_chunk_words             test_arena_at_its_bound
    rc_rans_encode_scratch_bytes    test_arena_at_its_bound
    rc_rans_encode_chunks           test_encoder_chunk_by_chunk
    rc_rans_compact                 test_encoder_chunk_by_chunk
    rc_rans_decode_chunks           test_decoder_routes_and_store_paths
    rc_rans_encode_host             test_one_chunk_is_the_single_stream
    rc_rans_decode_host             test_one_chunk_is_the_single_stream
"""
import numpy as np
import pytest
import torch

import codec_ref as C
import entropy_oracle as E
import rans_ref as R
from realcamnet_amd import _lib, bitstream
from test_codec_gpu import cu_count, knob

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
# route -> (dec_lds knob, rows of 1000 entries added in front of the edge rows)
ROUTES = {"tables in LDS": (1, 0), "in-kernel fall-back (rows do not fit the LDS)": (1, 40), "global kernel (dec_lds = 0)": (0, 0)}


def lib_tables(t):
    return bitstream.Tables(t["_quantized_cdf"], t["_cdf_length"], t["_offset"], "cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def encode_chunked(sym, idx, tables, chunk):
    return bitstream.encode(dev(sym), dev(idx), tables, "chunked", chunk)


def decode_chunked(blob, idx, tables):
    got = bitstream.Decoder(blob, tables, "cuda", "chunked").decode(dev(idx))
    torch.cuda.synchronize()
    return got.cpu().numpy()


def assert_symbols(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad.size), len(want), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def assert_chunks(blob, sym, idx, rows, chunk, what, which=None):
    """The container's header and size table are consistent and every chunk (or those in `which`) is the reference's stream of that chunk's symbols."""
    n, ch, streams = R.split_container(blob)
    assert n == len(sym) and ch == chunk, (what, n, ch)
    for c in (range(len(streams)) if which is None else which):
        want = R.encode(sym[c * chunk:(c + 1) * chunk], idx[c * chunk:(c + 1) * chunk], rows)
        assert streams[c] == want, (what, "chunk", c, "of", len(streams), len(streams[c]), len(want))
    return streams


def route_tables(rows_added):
    g = E.gc_update(E.get_scale_table())
    t = R.append_tables(C.big_tables(g, rows_added, 1000) if rows_added else g, R.edge_tables())
    fits = int(t["_cdf_length"].sum()) <= 32 * 1024                                   # kDecLdsEntries
    assert fits == (rows_added == 0)
    return t, 64 + rows_added


# ---- a. the encoder, chunk by chunk -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", R.ENC_CHUNKS)
def test_encoder_chunk_by_chunk(hip, chunk):
    """Every chunk of the container is rans_ref.encode of that chunk's symbols, the size table and the total length fit, and the container decodes to the symbols: chunk
    counts 1, 63, 64, 65, 129 with a last chunk of 1 symbol, chunk - 1 symbols and a full one (rans_ref.encoder_cases)."""
    e = R.edge_tables()
    rows, tables = R.Rows(e), lib_tables(e)
    sym, idx, calls = R.sliced(R.encoder_cases(chunk), R.SEEDS["encoder"] + chunk)
    R.assert_covered(sym, idx, rows)
    for start, n in calls:
        s, i = sym[start:start + n], idx[start:start + n]
        blob = encode_chunked(s, i, tables, chunk)
        assert_chunks(blob, s, i, rows, chunk, (chunk, n))
        assert_symbols(decode_chunked(blob, i, tables), s, (chunk, n))


# ---- b. one chunk --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_chunk_is_the_single_stream(hip):
    """chunk == n: the payload is the host coder's "compressai" stream and the reference's single stream, and the host decoder reads it."""
    e = R.edge_tables()
    rows, tables, host_tables = R.Rows(e), lib_tables(e), bitstream.Tables(e["_quantized_cdf"], e["_cdf_length"], e["_offset"], "cpu")
    sym, idx, calls = R.sliced(R.ONE_CHUNK_NS, R.SEEDS["one_chunk"])
    R.assert_covered(sym, idx, rows)
    for start, n in calls:
        s, i = sym[start:start + n], idx[start:start + n]
        streams = assert_chunks(encode_chunked(s, i, tables, n), s, i, rows, n, ("one chunk", n))
        assert len(streams) == 1
        assert streams[0] == bitstream.encode(torch.from_numpy(s), torch.from_numpy(i), host_tables, "compressai"), n
        got = bitstream.Decoder(streams[0], host_tables, "cpu", "compressai").decode(torch.from_numpy(i))
        assert_symbols(got.numpy(), s, ("host decoder", n))


# ---- c. the decoder: every route and both store paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_decoder_routes_and_store_paths(hip, route):
    """The full edge symbols (8-nibble escapes included) come back on the three routes, at chunk lengths of 0, 1, 2 and 3 mod 4, into torch's own (16-byte aligned)
    output and, through the C entry, into a d_symbols 4 bytes past a 16-byte boundary inside a larger tensor whose values in front and behind stay untouched: with
    chunk % 4 == 0 the first takes the LDS kernel's 16-byte stores and the second its element stores."""
    dec_lds, rows_added = ROUTES[route]
    t, first = route_tables(rows_added)
    rows, tables = R.Rows(t), lib_tables(t)
    sym, idx, calls = R.sliced([n for _, n in R.DEC_CASES], R.SEEDS["decoder"], tables=rows, first_row=first)
    R.assert_covered(sym, idx, rows, first_row=first)
    with knob(hip, b"dec_lds", dec_lds, 1):
        for (chunk, n), (start, n_) in zip(R.DEC_CASES, calls):
            assert n == n_
            s, i = sym[start:start + n], idx[start:start + n]
            blob = encode_chunked(s, i, tables, chunk)
            streams = assert_chunks(blob, s, i, rows, chunk, (route, chunk, n), which=(0, -(-n // chunk) - 1))
            assert_symbols(decode_chunked(blob, i, tables), s, (route, chunk, n, "aligned"))
            # the C entry, d_symbols = buf + 5: 4 bytes past a 16-byte boundary
            payload = dev(np.frombuffer(b"".join(streams), dtype=np.uint8).copy())
            offsets = dev(np.concatenate([[0], np.cumsum([len(x) for x in streams])[:-1]]).astype(np.int64))
            d_idx = dev(i)
            buf = torch.full((n + 16,), SENTINEL, dtype=torch.int32, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            out = buf[5:5 + n]
            assert out.data_ptr() % 16 == 4
            assert hip.rc_rans_decode_chunks(payload.data_ptr(), payload.numel(), offsets.data_ptr(), d_idx.data_ptr(), n, chunk, tables.cdf.data_ptr(),
                                             tables.cdf.shape[1], tables.cdf.shape[0], tables.sizes.data_ptr(), tables.offsets.data_ptr(), out.data_ptr(),
                                             err.data_ptr(), None) == 0
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert int(err.item()) == 0, (route, chunk, n)
            assert_symbols(got[5:5 + n], s, (route, chunk, n, "4 bytes past a 16-byte boundary"))
            assert (got[:5] == SENTINEL).all() and (got[5 + n:] == SENTINEL).all(), (route, chunk, n, got[:5], got[5 + n:])


# ---- d. several chunks per wave -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", R.LANE_CHUNKS)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["2 lanes", "3 lanes", "64 lanes"])
def test_several_chunks_per_wave(hip, which, chunk):
    """The LDS decoder gives a wave lanes = ceil(n_chunks / (2 CUs)) chunks, 64 at the most: the smallest chunk counts with 2, 3 and 64 lanes (513, 1025 and 32257
    on 256 CUs) decode to the encoded symbols, and the container is the reference's on the first chunk, the last and a seeded sample of 64."""
    cu = cu_count()
    lanes, n_chunks = R.lane_cases(cu)[which]
    assert R.lanes_for(n_chunks, cu) == lanes == (2, 3, 64)[which] and R.lanes_for(n_chunks - 1, cu) == lanes - 1
    e = R.edge_tables()
    rows, tables = R.Rows(e), lib_tables(e)
    n = (n_chunks - 1) * chunk + 1
    sym, idx = R.edge_symbols(n, R.SEEDS["lanes"] + 100 * chunk + lanes)
    R.assert_covered(sym, idx, rows)
    blob = encode_chunked(sym, idx, tables, chunk)
    sample = sorted({0, n_chunks - 1} | set(np.random.default_rng(lanes).choice(n_chunks, 64, replace=False).tolist()))
    streams = assert_chunks(blob, sym, idx, rows, chunk, (lanes, chunk), which=sample)
    assert len(streams) == n_chunks
    assert_symbols(decode_chunked(blob, idx, tables), sym, (lanes, chunk))


# ---- e. the arena at its bound ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", R.ARENA_CHUNKS)
def test_arena_at_its_bound(hip, chunk):
    """rc_rans_encode_chunks on worst_case symbols (52 bits each) into a word arena of rc_rans_chunk_words(chunk) words a chunk, pre-filled with a sentinel and with guard
    words around it and behind the scratch of rc_rans_encode_scratch_bytes: nbytes is the reference's, each stream sits at the end of its chunk's region, every word in
    front of it and every guard word is still the sentinel."""
    e = R.edge_tables()
    rows, tables = R.Rows(e), lib_tables(e)
    n = 4 * chunk - (chunk > 1)                                    # three full chunks and one of chunk - 1 symbols (chunk 1: four of one)
    n_chunks = -(-n // chunk)
    sym, idx = R.worst_case(n)
    assert R.escape_classes(sym, idx, rows) == {(8, -1): n}
    cap = hip.rc_rans_chunk_words(chunk)
    assert cap == 2 * chunk + 8
    guard = 64
    arena = torch.full((guard + n_chunks * cap + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    scratch_bytes = hip.rc_rans_encode_scratch_bytes(n, chunk)
    assert scratch_bytes == n_chunks * chunk * 18 + 16
    scratch = torch.full(((scratch_bytes + 7) // 8 + guard,), -1, dtype=torch.int64, device="cuda")
    nbytes = torch.full((guard + n_chunks + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    d_sym, d_idx = dev(sym), dev(idx)
    assert hip.rc_rans_encode_chunks(d_sym.data_ptr(), d_idx.data_ptr(), n, chunk, tables.cdf.data_ptr(), tables.cdf.shape[1], tables.cdf.shape[0],
                                     tables.sizes.data_ptr(), tables.offsets.data_ptr(), arena[guard:].data_ptr(), nbytes[guard:].data_ptr(), scratch.data_ptr(),
                                     None) == 0
    torch.cuda.synchronize()
    words, sizes = arena.cpu().numpy().view(np.uint32), nbytes.cpu().numpy()
    assert (words[:guard] == SENTINEL).all() and (words[guard + n_chunks * cap:] == SENTINEL).all()
    assert (sizes[:guard] == SENTINEL).all() and (sizes[guard + n_chunks:] == SENTINEL).all()
    assert (scratch.cpu().numpy()[(scratch_bytes + 7) // 8:] == -1).all()
    for c in range(n_chunks):
        want = R.encode(sym[c * chunk:(c + 1) * chunk], idx[c * chunk:(c + 1) * chunk], rows)
        assert int(sizes[guard + c]) == len(want), (chunk, c, int(sizes[guard + c]), len(want))
        region = words[guard + c * cap:guard + (c + 1) * cap]
        nw = len(want) // 4
        assert nw <= cap
        assert region[cap - nw:].astype("<u4").tobytes() == want, (chunk, c)
        assert (region[:cap - nw] == SENTINEL).all(), (chunk, c)


# ---- f. errors that cannot read out of bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_bad_index_and_long_escape_are_errors(hip, route):
    """A CDF index of n_cdfs or -1 at the first symbol, at the last and inside one chunk of many: the encoder raises "CDF index out of range" and the decoder, given the
    intact container, reports the same (error 1).  The reference's well-formed stream with one 9-nibble escape, in a container of correct sizes, ends in "truncated or
    corrupt" (error 2).  Every stream is whole and every offset valid."""
    dec_lds, rows_added = ROUTES[route]
    t, first = route_tables(rows_added)
    rows, tables = R.Rows(t), lib_tables(t)
    n, chunk = 2000, 250
    sym, idx = R.edge_symbols(n, R.SEEDS["errors"], tables=rows, first_row=first)
    R.assert_covered(sym, idx, rows, first_row=first)
    n_cdfs = len(rows.rows)
    with knob(hip, b"dec_lds", dec_lds, 1):
        blob = encode_chunked(sym, idx, tables, chunk)
        assert_symbols(decode_chunked(blob, idx, tables), sym, route)
        for at in (0, n - 1, 3 * chunk + 77):
            for value in (n_cdfs, -1):
                bad = idx.copy()
                bad[at] = value
                with pytest.raises(_lib.HipError, match="CDF index out of range"):
                    encode_chunked(sym, bad, tables, chunk)
                with pytest.raises(_lib.HipError, match="CDF index out of range"):
                    decode_chunked(blob, bad, tables)
            long = [int(s) for s in sym]
            long[at] = (1 << 31) + 400 + rows.offs[int(idx[at])]
            streams = [R.encode(long[c:c + chunk], idx[c:c + chunk], rows, max_nibbles=9) for c in range(0, n, chunk)]
            with pytest.raises(_lib.HipError, match="truncated or corrupt"):
                decode_chunked(R.container(n, chunk, streams), idx, tables)
        assert_symbols(decode_chunked(blob, idx, tables), sym, (route, "after the errors"))


# ---- g. a second run -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_second_run_gives_the_same_bytes(hip):
    e = R.edge_tables()
    tables = lib_tables(e)
    sym, idx = R.edge_symbols(5000, R.SEEDS["second_run"])
    R.assert_covered(sym, idx, e)
    for chunk in (33, 250):
        first = encode_chunked(sym, idx, tables, chunk)
        assert encode_chunked(sym, idx, tables, chunk) == first
        a, b = decode_chunked(first, idx, tables), decode_chunked(first, idx, tables)
        assert_symbols(a, sym, chunk)
        assert np.array_equal(a, b)


# ---- h. past the grid cap of the preparation kernel ------------------------------------------------------------------------------------------------------------------------
def test_preparation_kernel_past_its_grid_cap(hip):
    """prepare_kernel launches at most 65535 blocks of 256 threads and strides over the rest: 65535 * 256 + 77 symbols (a covered input of 4999 symbols repeated; 4999
    and 2048 are coprime, so no two chunks of the sample start at the same place in it) decode to themselves, and the first chunk, the last two (the last holds the 77
    symbols of the second stride) and a seeded sample of 60 are the reference's."""
    e = R.edge_tables()
    rows, tables = R.Rows(e), lib_tables(e)
    base_sym, base_idx = R.edge_symbols(4999, R.SEEDS["grid_cap"])
    R.assert_covered(base_sym, base_idx, rows)
    n, chunk = 65535 * 256 + 77, 2048
    sym, idx = np.resize(base_sym, n), np.resize(base_idx, n)
    n_chunks = -(-n // chunk)
    blob = encode_chunked(sym, idx, tables, chunk)
    assert (n_chunks - 1) * chunk < 65535 * 256 < n                      # the symbols of the second stride lie in the last chunk
    sample = sorted({0, n_chunks - 2, n_chunks - 1} | set(np.random.default_rng(5).choice(n_chunks, 60, replace=False).tolist()))
    assert_chunks(blob, sym, idx, rows, chunk, "past the grid cap", which=sample)
    d_idx = dev(idx)
    got = bitstream.Decoder(blob, tables, "cuda", "chunked").decode(d_idx)
    assert torch.equal(got, dev(sym))
