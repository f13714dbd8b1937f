"""tests/second_model.c behind ctypes: compiled with gcc into a temporary directory on first use.

second(read, ref, scoring, mask_len) -> (score1, ref_end1, score2, ref_end2), what ssw_align reports for the pair
(DESIGN, "Second-best alignment"); mask_len_of(read) is Aligner.align's maskLen (ssw_wrap.py:198-201)."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CODE = np.full(256, 4, np.uint8)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _k
_lib = None


def _load():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="second_model_")
        atexit.register(shutil.rmtree, tmp, True)
        so = os.path.join(tmp, "libsecond_model.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(_HERE, "second_model.c")])
        _lib = ctypes.CDLL(so)
        _lib.second_model.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 5 + [
            ctypes.c_void_p]
        _lib.second_model.restype = None
    return _lib


def codes(seq):
    """One code per letter: A C G T = 0..3, anything else 4."""
    return _CODE[np.frombuffer(seq.encode("latin-1"), np.uint8)] if seq else np.zeros(0, np.uint8)


def mask_len_of(read):
    return len(read) // 2 if len(read) > 30 else 15


def second(read, ref, scoring, mask_len):
    """scoring: (match, mismatch, gap_open, gap_extend)"""
    lib = _load()
    r, t = np.ascontiguousarray(codes(read)), np.ascontiguousarray(codes(ref))
    out = np.zeros(4, np.int32)
    lib.second_model(r.ctypes.data, len(r), t.ctypes.data, len(t), *[int(v) for v in scoring], int(mask_len), out.ctypes.data)
    return tuple(int(v) for v in out)


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def template(ladder, t):
    """Template t of a ladder in db order (u=1 fwd, u=1 rc, u=2 fwd, ...); max_units 0: the plain reference."""
    prefix, repeat, suffix, mu = ladder
    if mu == 0:
        return prefix
    s = prefix + repeat * (t // 2 + 1) + suffix
    return "".join(_COMP[c] for c in reversed(s)) if t % 2 else s


_golden = None


def golden():
    """tests/golden/sw_second.npz (tools/gen_golden_second.py) as a dict: per item cls, ladder, template, reads, refs (the
    template's letters), scoring (4 ints), mask_len, expect (the reference's score1, ref_end1, score2, ref_end2); ladders
    and meta.  Loaded once and shared: nobody changes it."""
    global _golden
    if _golden is None:
        import json
        z = np.load(os.path.join(_HERE, "golden", "sw_second.npz"))
        meta = json.loads(str(z["meta"]))
        blob, off = z["reads"].tobytes().decode(), z["read_off"]
        g = {k: z[k] for k in ("cls", "ladder", "template", "scoring", "mask_len", "expect")}
        g["reads"] = [blob[off[k]:off[k + 1]] for k in range(len(off) - 1)]
        g["ladders"] = [tuple(l) for l in meta["ladders"]]
        g["refs"] = [template(g["ladders"][l], t) for l, t in zip(g["ladder"], g["template"])]
        g["meta"] = meta
        _golden = g
    return _golden
