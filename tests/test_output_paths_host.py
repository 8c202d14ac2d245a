"""CPU: the coverage table of test_output_paths_gpu.py against the header and the kernel sources."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP = '#include "rgb_strip.hpp"'
ENCODERS = {"rc_rgb_encode", "rc_yuv_encode"}        # their own access rules (raw_format.hip, yuv_encode.hip / yuv_surface.hip): in the table by name


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def frame_entries():
    """The entry points that read planar frames through rgb_strip.hpp: declared in the header with a device source (`const void* d_src`) and
    defined in a translation unit that includes the strip reader; and the two encoders."""
    header = re.sub(r"/\*.*?\*/", "", read("include", "realcam_hip.h"), flags=re.S)
    reads_frames = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(\s*const void\*\s*d_src\b", header))
    csrc = os.path.join(ROOT, "realcamnet_amd", "csrc")
    defined = set()
    for tu in sorted(os.listdir(csrc)):
        if tu.endswith(".hip"):
            src = read("realcamnet_amd", "csrc", tu)
            if STRIP in src:
                defined |= set(re.findall(r"^int (rc_[a-z0-9_]+)\(", src, flags=re.M))
    assert ENCODERS <= reads_frames
    return (defined & reads_frames) | ENCODERS


def test_coverage_table_names_every_entry_and_tests_that_exist():
    entries = frame_entries()
    assert {"rc_lut3d", "rc_warp", "rc_resize", "rc_frame_stats", "rc_sharpen", "rc_tone_apply"} <= entries and len(entries) >= 8, sorted(entries)
    gpu = read("tests", "test_output_paths_gpu.py")
    doc = gpu.split('"""')[1]
    rows = re.findall(r"^\s{4}(rc_[a-z0-9_]+)\s+(\S+)\s+(?:(test_[a-z0-9_]+\.py)::)?(test_[a-z0-9_]+)\s*$", doc, flags=re.M)
    assert len(rows) >= len(entries)
    named = {r[0] for r in rows}
    assert named == entries, (sorted(entries - named), sorted(named - entries))
    tests_of = {}
    for entry, paths, module, test in rows:
        assert paths and all(re.fullmatch(r"[ve-]{2}|walk|guard|refusal", p) for p in paths.split(",")), (entry, paths)
        module = module or "test_output_paths_gpu.py"
        if module not in tests_of:
            tests_of[module] = set(re.findall(r"^def (test_[a-z0-9_]+)\(", read("tests", module), flags=re.M))
        assert test in tests_of[module], (entry, module, test)
    # every test of the module is in the table: none runs unlisted
    assert tests_of["test_output_paths_gpu.py"] == {r[3] for r in rows if not r[2]}
    # the module keeps its word: no skip, no expected failure, no tolerance
    body = gpu.split('"""', 2)[2]
    assert not re.search(r"\b(skip|skipif|xfail|allclose|isclose|atol|rtol)\b", body)
