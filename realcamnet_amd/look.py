"""Colour looks for forward_mosaic's outputs: `Lut3D`, a 3D LUT in the `.cube` format that grading tools, cameras and monitors exchange,
applied by ops.lut3d with tetrahedral interpolation (include/realcam_hip.h, rc_lut3d).

Pure Python and NumPy: parsing and validation raise ValueError / TypeError and never touch the GPU or the library.
"""
from __future__ import annotations

import hashlib
import math
import os
from typing import Optional

import numpy as np

from . import _lib

MIN_SIZE = _lib.RC_LUT3D_MIN_SIZE
MAX_SIZE = _lib.RC_LUT3D_MAX_SIZE
_KEYWORDS = ("TITLE", "LUT_3D_SIZE", "LUT_1D_SIZE", "DOMAIN_MIN", "DOMAIN_MAX", "LUT_1D_INPUT_RANGE", "LUT_3D_INPUT_RANGE")


class Lut3D:
    """An immutable 3D LUT on the unit cube.

    table   array-like (N, N, N, 3) fp32, 2 <= N <= 65, every value finite: table[ib, ig, ir, :] is the output (R, G, B) at grid node
            (ir, ig, ib) -- R varies fastest, the order of a .cube file's rows.
    title   the file's TITLE, kept for to_cube(); it takes no part in equality.
    Equal and hashed by content (the size and a digest of the bytes, computed once): a Lut3D keys the device-table cache of ops.lut3d
    and sits inside the frozen Output.
    """

    __slots__ = ("_table", "_n", "_digest", "_title")

    def __init__(self, table, title: Optional[str] = None):
        if title is not None and not isinstance(title, str):
            raise TypeError(f"Lut3D.title must be None or a str, got {type(title).__name__}")
        if title is not None and ('"' in title or "\n" in title or "\r" in title):
            raise ValueError("Lut3D.title must not hold a double quote or a line break (it is written as TITLE \"...\")")
        if isinstance(table, (str, bytes)) or table is None:
            raise TypeError(f"Lut3D.table must be array-like of shape (N, N, N, 3), got {type(table).__name__}")
        try:
            a = np.asarray(table)
        except Exception as e:                                           # ragged lists and the like
            raise TypeError(f"Lut3D.table must be array-like of shape (N, N, N, 3): {e}") from None
        if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"Lut3D.table must hold real numbers, got dtype {a.dtype}")
        if a.ndim != 4 or a.shape[3] != 3 or not (a.shape[0] == a.shape[1] == a.shape[2]):
            raise ValueError(f"Lut3D.table must have shape (N, N, N, 3), got {a.shape}")
        n = int(a.shape[0])
        if not MIN_SIZE <= n <= MAX_SIZE:
            raise ValueError(f"Lut3D: size {n} outside {MIN_SIZE} .. {MAX_SIZE}")
        with np.errstate(over="ignore"):
            t = np.array(a, dtype=np.float32, order="C", copy=True)      # the private copy; a double beyond fp32 becomes inf and is refused
        if not np.isfinite(t).all():
            raise ValueError("Lut3D.table must be finite (no NaN, no infinity, nothing beyond fp32)")
        t.flags.writeable = False
        object.__setattr__(self, "_table", t)
        object.__setattr__(self, "_n", n)
        object.__setattr__(self, "_digest", hashlib.sha256(t.tobytes()).digest())
        object.__setattr__(self, "_title", title)

    def __setattr__(self, name, value):
        raise AttributeError("Lut3D is immutable")

    def __delattr__(self, name):
        raise AttributeError("Lut3D is immutable")

    @property
    def table(self) -> np.ndarray:
        """The (N, N, N, 3) fp32 table, read-only."""
        return self._table

    @property
    def size(self) -> int:
        return self._n

    @property
    def title(self) -> Optional[str]:
        return self._title

    def __eq__(self, other):
        if not isinstance(other, Lut3D):
            return NotImplemented
        return self._n == other._n and self._digest == other._digest

    def __hash__(self):
        return hash((self._n, self._digest))

    def __repr__(self):
        return f"Lut3D(size={self._n}, title={self._title!r}, sha256={self._digest.hex()[:12]})"

    def packed(self) -> np.ndarray:
        """The table as rc_lut3d reads it: (N^3, 4) fp32, entry ir + N (ig + N ib) = R, G, B and a zero pad float."""
        out = np.zeros((self._n ** 3, 4), dtype=np.float32)
        out[:, :3] = self._table.reshape(-1, 3)
        return out

    @classmethod
    def identity(cls, n: int, title: Optional[str] = None) -> "Lut3D":
        """The look that changes nothing inside [0, 1]: node (ir, ig, ib) holds (ir, ig, ib) / (n - 1), divided in double, rounded to fp32 once."""
        if not isinstance(n, int) or isinstance(n, bool):
            raise TypeError(f"Lut3D.identity: size must be an int, got {type(n).__name__}")
        if not MIN_SIZE <= n <= MAX_SIZE:
            raise ValueError(f"Lut3D: size {n} outside {MIN_SIZE} .. {MAX_SIZE}")
        g = np.arange(n, dtype=np.float64) / np.float64(n - 1)
        t = np.empty((n, n, n, 3), dtype=np.float64)
        t[..., 0] = g[None, None, :]
        t[..., 1] = g[None, :, None]
        t[..., 2] = g[:, None, None]
        return cls(t.astype(np.float32), title)

    def to_cube(self) -> str:
        """The look as .cube text; from_cube of it equals this look bit for bit (every float is written with repr's exact precision)."""
        head = ([f'TITLE "{self._title}"'] if self._title is not None else []) + [f"LUT_3D_SIZE {self._n}", "DOMAIN_MIN 0.0 0.0 0.0", "DOMAIN_MAX 1.0 1.0 1.0"]
        rows = self._table.reshape(-1, 3).astype(np.float64).tolist()    # fp32 -> double is exact, and repr of a double parses back to it
        return "\n".join(head + [f"{r!r} {g!r} {b!r}" for r, g, b in rows]) + "\n"

    @classmethod
    def from_cube(cls, path_or_text) -> "Lut3D":
        """Parse a .cube file (a path), or its text (a str with a line break in it).

        Accepted: `#` comments and blank lines; before the data and in any order TITLE "...", LUT_3D_SIZE N, DOMAIN_MIN 0 0 0 and
        DOMAIN_MAX 1 1 1; then exactly N^3 rows of three floats, R fastest.  Refused with a ValueError that names the line: LUT_1D_SIZE,
        any other domain or keyword, a missing or repeated size, a wrong row count, a non-finite or unparsable number, N outside 2 .. 65."""
        if isinstance(path_or_text, os.PathLike) or (isinstance(path_or_text, str) and "\n" not in path_or_text and "\r" not in path_or_text):
            with open(path_or_text, "r", encoding="utf-8-sig") as f:
                text = f.read()
        elif isinstance(path_or_text, str):
            text = path_or_text
        else:
            raise TypeError(f"Lut3D.from_cube: expected a path or the file's text, got {type(path_or_text).__name__}")
        n = title = None
        seen = set()
        data, need, first_row = [], 0, 0
        for no, raw in enumerate(text.splitlines(), 1):
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            tok = line.split()
            key = tok[0].upper()
            if key in _KEYWORDS:
                if data:
                    raise ValueError(f".cube line {no}: keyword {key} after the first data row (line {first_row})")
                if key in seen:
                    raise ValueError(f".cube line {no}: {key} is repeated")
                seen.add(key)
                if key == "TITLE":
                    rest = line[len(tok[0]):].strip()
                    if len(rest) < 2 or rest[0] != '"' or rest[-1] != '"' or '"' in rest[1:-1]:
                        raise ValueError(f".cube line {no}: TITLE must be one string in double quotes")
                    title = rest[1:-1]
                elif key == "LUT_3D_SIZE":
                    if len(tok) != 2 or not tok[1].isdigit():
                        raise ValueError(f".cube line {no}: LUT_3D_SIZE takes one integer, got {line!r}")
                    n = int(tok[1])
                    if not MIN_SIZE <= n <= MAX_SIZE:
                        raise ValueError(f".cube line {no}: LUT_3D_SIZE {n} outside {MIN_SIZE} .. {MAX_SIZE}")
                    need = n ** 3
                elif key in ("DOMAIN_MIN", "DOMAIN_MAX"):
                    want = 0.0 if key == "DOMAIN_MIN" else 1.0
                    try:
                        vals = [float(v) for v in tok[1:]]
                    except ValueError:
                        vals = []
                    if len(tok) != 4 or vals != [want] * 3:
                        raise ValueError(f".cube line {no}: only the unit domain is supported ({key} {want:g} {want:g} {want:g}), got {line!r}")
                elif key == "LUT_1D_SIZE":
                    raise ValueError(f".cube line {no}: LUT_1D_SIZE: 1D (shaper) LUTs are not supported")
                else:
                    raise ValueError(f".cube line {no}: {key} (a non-unit input range) is not supported")
                continue
            if not _is_number(tok[0]) and (tok[0][0].isalpha() or tok[0][0] == "_"):
                raise ValueError(f".cube line {no}: unknown keyword {tok[0]!r}")
            if n is None:
                raise ValueError(f".cube line {no}: a data row before LUT_3D_SIZE (the size is missing)")
            if len(tok) != 3:
                raise ValueError(f".cube line {no}: a data row holds three numbers, got {line!r}")
            try:
                row = (float(tok[0]), float(tok[1]), float(tok[2]))
            except ValueError:
                raise ValueError(f".cube line {no}: unparsable number in {line!r}") from None
            if not (math.isfinite(row[0]) and math.isfinite(row[1]) and math.isfinite(row[2])):
                raise ValueError(f".cube line {no}: non-finite number in {line!r}")
            if len(data) == need:
                raise ValueError(f".cube line {no}: more than {need} data rows for LUT_3D_SIZE {n}")
            if not data:
                first_row = no
            data.append(row)
        if n is None:
            raise ValueError(f".cube: LUT_3D_SIZE is missing (end of text after line {len(text.splitlines())})")
        if len(data) != need:
            raise ValueError(f".cube: {len(data)} data rows up to the last line ({len(text.splitlines())}), LUT_3D_SIZE {n} needs {need}")
        with np.errstate(over="ignore"):
            t = np.asarray(data, dtype=np.float64).astype(np.float32)
        bad = np.argwhere(~np.isfinite(t))
        if len(bad):
            raise ValueError(f".cube data row {int(bad[0][0]) + 1} (from line {first_row} on): a number beyond fp32")
        return cls(t.reshape(n, n, n, 3), title)


def _is_number(s: str) -> bool:
    try:
        float(s)
        return True
    except ValueError:
        return False
