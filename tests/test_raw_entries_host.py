"""CPU: the refusals the six sensor-stage entry points share (csrc/raw_row.hpp: raw_source, raw_frames, raw_pitch, all_zero) -- rc_raw_ingest_fmt,
rc_raw_defects, rc_raw_calibrate, rc_raw_hdr_merge, rc_raw_temporal and rc_raw_quad.  One function forms these messages for six callers, so every
case asserts the return code, the substring the entry's own table matches, and that the message opens with the entry's own name.  The frames are
the smallest the six tables use (h = 4, w = 8) at addresses that are never dereferenced: nothing is enqueued."""
import ctypes as C

import pytest

from realcamnet_amd import _lib

FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before anything is enqueued
PREV, DST = FAKE + (1 << 16), FAKE + (1 << 17)       # rc_raw_temporal's state and destination: apart, so that no case is an overlap
U16, F32, MIPI10, MIPI12 = _lib.RC_RAW_U16, _lib.RC_RAW_F32, _lib.RC_RAW_MIPI10, _lib.RC_RAW_MIPI12


def _ints(n, v):
    return (C.c_int32 * n)(*v)


# Each entry: called with the shared keywords (src, dst, dst_pitch, b, h, w, the format's fields, the desc's reserved words) and valid values
# for everything else.  The mosaic is (2h, 2w) = (8, 16): a u16 row is 32 bytes, a RAW10 row 20, a RAW12 row 24.
def _ingest(lib, f, kw):
    return lib.rc_raw_ingest_fmt(kw["src"], C.byref(f), kw["dst"], FAKE, _lib.RC_F32, kw["b"], kw["h"], kw["w"], 16, 16, 4, 4, None)


def _defects(lib, f, kw):
    d = _lib.DefectDesc(flags=3, hot_abs=1.0, hot_rel=0.0, cold_abs=1.0, cold_rel=0.0, reserved=_ints(3, kw["reserved"][:3]))
    return lib.rc_raw_defects(kw["src"], C.byref(f), C.byref(d), FAKE, 4, kw["dst"], kw["dst_pitch"], FAKE, kw["b"], kw["h"], kw["w"], None)


def _calibrate(lib, f, kw):
    ramp = (C.c_float * 16)(*range(16))
    d = _lib.CalibDesc(flags=3, knots=16, cell=8, curve_x=ramp, curve_y=ramp, gains=(C.c_float * 4)(1.0, 1.0, 1.0, 1.0), clip_lo=0.0, clip_hi=1.0,
                       reserved=_ints(3, kw["reserved"][:3]))
    return lib.rc_raw_calibrate(kw["src"], C.byref(f), C.byref(d), FAKE, None, 0, kw["dst"], _lib.RC_F32, kw["dst_pitch"], kw["b"], kw["h"], kw["w"], None)


def _hdr(lib, f, kw):
    d = _lib.HdrDesc(exposures=3, flags=1, times=(C.c_float * 4)(1.0, 4.0, 16.0, 0.0), knee_lo=192.0, knee_hi=256.0, motion_abs=4.0, motion_rel=0.125,
                     exposure_stride_bytes=0, frame_stride_bytes=0, reserved=_ints(4, kw["reserved"]))
    return lib.rc_raw_hdr_merge(kw["src"], C.byref(f), C.byref(d), None, 0, kw["dst"], kw["dst_pitch"], kw["b"], kw["h"], kw["w"], None)


def _temporal(lib, f, kw):
    d = _lib.TemporalDesc(flags=0, noise_abs=4.0, noise_rel=0.03125, alpha=0.125, ramp=3.0, gain=0.0, reserved=_ints(4, kw["reserved"]))
    return lib.rc_raw_temporal(kw["src"], C.byref(f), C.byref(d), kw["prev"], kw["prev_pitch"], None, 0, kw["dst"], kw["dst_pitch"],
                               kw["b"], kw["h"], kw["w"], None)


def _quad(lib, f, kw):                                  # takes the mosaic's own size
    d = _lib.QuadDesc(mode=0, reserved=_ints(3, kw["reserved"][:3]))
    return lib.rc_raw_quad(kw["src"], C.byref(f), C.byref(d), kw["dst"], kw["dst_pitch"], kw["b"], 2 * kw["h"], 2 * kw["w"], None)


# name -> (the call, bytes per sample of its default destination, its default destination)
ENTRIES = {
    "rc_raw_ingest_fmt": (_ingest, None, FAKE),
    "rc_raw_defects": (_defects, 2, FAKE),
    "rc_raw_calibrate": (_calibrate, 4, FAKE),
    "rc_raw_hdr_merge": (_hdr, 4, FAKE),
    "rc_raw_temporal": (_temporal, 4, DST),
    "rc_raw_quad": (_quad, 2, FAKE),
}
STAGES = [e for e in ENTRIES if e != "rc_raw_ingest_fmt"]                          # the entries with a frame limit, a dst pitch and a desc

# What raw_source refuses, for every entry.
SOURCE = [
    ("storage 7", dict(storage=7), b"storage"), ("storage -1", dict(storage=-1), b"storage"),
    ("cfa 4", dict(cfa=4), b"cfa"), ("cfa -1", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"),
    ("width", dict(width=12), b"width"),
    ("line_bytes short (u16)", dict(line_bytes=30), b"line_bytes"), ("line_bytes short (RAW10)", dict(storage=MIPI10, line_bytes=19), b"line_bytes"),
    ("line_bytes short (RAW12)", dict(storage=MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("mipi base misaligned", dict(storage=MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=F32, src=FAKE + 2), b"misaligned"),
]
CASES = [(e, case, kw, msg) for e in ENTRIES for case, kw, msg in SOURCE]
# rc_raw_quad's width is a multiple of 4 before raw_source sees it: the RAW10 rule cannot be reached through it
CASES += [(e, "RAW10 2w % 4", dict(storage=MIPI10, w=7, width=14), b"RAW10") for e in ENTRIES if e != "rc_raw_quad"]
# raw_frames (rc_raw_ingest_fmt and rc_raw_quad word their own shape check: the same substring)
CASES += [(e, case, kw, b"bad shape") for e in ENTRIES for case, kw in (("empty", dict(h=0)), ("no frames", dict(b=0)))]
CASES += [(e, "too many frames", dict(b=65536), b"bad shape") for e in STAGES]
# raw_pitch for the destination, and all_zero for the desc
for e in STAGES:
    es = ENTRIES[e][1]
    CASES += [(e, "dst pitch short", dict(dst_pitch=16 * es - es), b"dst pitch"), (e, "dst pitch odd", dict(dst_pitch=16 * es + es // 2), b"dst pitch"),
              (e, "dst misaligned", dict(dst=ENTRIES[e][2] + es // 2), b"dst misaligned"),
              (e, "desc reserved", dict(reserved=(0, 0, 1, 0)), b"reserved")]
# raw_pitch for rc_raw_temporal's state: the name is an argument too
CASES += [("rc_raw_temporal", "prev pitch short", dict(prev_pitch=60), b"prev pitch"), ("rc_raw_temporal", "prev pitch odd", dict(prev_pitch=66), b"prev pitch"),
          ("rc_raw_temporal", "prev misaligned", dict(prev=PREV + 2), b"prev misaligned")]


@pytest.mark.parametrize("entry,case,kwargs,msg", CASES, ids=[f"{e}-{c}" for e, c, _, _ in CASES])
def test_shared_refusals_name_their_entry(entry, case, kwargs, msg):
    call, _, dst = ENTRIES[entry]
    kw = dict(src=FAKE, dst=dst, dst_pitch=0, prev=PREV, prev_pitch=0, b=1, h=4, w=8, storage=U16, cfa=0, line_bytes=0, width=0, reserved=(0, 0, 0, 0),
              fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(64.0, 64.0, 64.0, 64.0),
                           white=1023.0, reserved=_ints(4, kw["fmt_reserved"]))
    lib = _lib.load()
    assert call(lib, f, kw) == -1, (entry, case)                                  # RC_ERR_INVALID
    err = lib.rc_last_error()
    assert err.startswith(entry.encode() + b":") and msg in err, (entry, case, err)
