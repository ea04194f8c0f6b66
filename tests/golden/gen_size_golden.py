#!/usr/bin/env python3
"""Generate tests/golden/size_cases.json from the reference compiled in
oracle/_ref (run from the repo root where the reference sources exist):

    make -C oracle ref && python3 tests/golden/gen_size_golden.py

For every case of tests/size_limit_cases.py (frames whose size lands exactly
on a limit) the compiled reference runs the case's call loop; recorded are the
return value of every call and one sha256 over what size_limit_cases.trace
observes after every call (return value, frame bytes, identifier, sequence
number, model size, work buffer).  Values and digests only; the 16 MB cases
are recorded the same way.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg, REF_PATH, ORC_PATH  # noqa: E402

api = load_pkg().cmpapi
import size_limit_cases as lc  # noqa: E402


def orc_ext():
    lib = ctypes.CDLL(ORC_PATH, mode=ctypes.RTLD_LOCAL)
    lib.orc_select_rice_k.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_void_p]
    lib.orc_select_rice_k.restype = ctypes.c_uint32
    return lib


def main():
    ref = api.CmpLib(REF_PATH)
    orc = api.CmpLib(ORC_PATH)
    ext = orc_ext()
    cases = {}
    for name, case in lc.cpu_catalogue(orc).items():
        lc.self_check(orc, case, ext)
        tr = lc.trace(ref, case, ext)
        assert lc.trace(orc, case, ext) == tr, name
        cases[name] = dict(returns=[t[0] for t in tr], digest=lc.trace_digest(tr))
    with open(os.path.join(HERE, "size_cases.json"), "w") as f:
        json.dump(dict(generator="tests/golden/gen_size_golden.py", produced_by="oracle/_ref/libref.so",
                       note="digest = sha256(repr(tests.size_limit_cases.trace(lib, case)))", cases=cases), f,
                  indent=0)
    print("size cases:", len(cases))


if __name__ == "__main__":
    main()
