"""Generates tests/golden/fits/*.fits -- the files libcfitsio writes for the inputs of tests/test_fits.py.

PROVENANCE: written by libcfitsio itself (the library under the reference's CCfits calls, densitymaps.cpp:549-583),
through the call sequence CCfits issues for FITS(name, FLOAT_IMG, 2, naxes); pHDU().write(...); addKey(...)*.  The
tests compare this repository's FITS writers with these bytes, so they run where libcfitsio is not installed.

Run from the repository root on a machine with libcfitsio:  python tests/golden/make_fits_golden.py [path/to/libcfitsio.so]
"""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import test_fits  # noqa: E402  (the inputs)


def cfitsio_write(L, path, img, keys):
    f, st = C.c_void_p(), C.c_int(0)
    L.ffinit(C.byref(f), path.encode(), C.byref(st))
    naxes = (C.c_long * 2)(img.shape[1], img.shape[0])
    L.ffcrim(f, -32, 2, naxes, C.byref(st))
    flat = np.ascontiguousarray(img, np.float32).reshape(-1)
    L.ffppr(f, 42, C.c_longlong(1), C.c_longlong(flat.size), flat.ctypes.data_as(C.c_void_p), C.byref(st))
    for name, val, comm in keys:
        if isinstance(val, int):
            v = C.c_int(val)
            L.ffuky(f, 31, name.encode(), C.byref(v), comm.encode(), C.byref(st))
        else:
            v = C.c_double(val)
            L.ffuky(f, 82, name.encode(), C.byref(v), comm.encode(), C.byref(st))
    L.ffclos(f, C.byref(st))
    assert st.value == 0
    print(path, os.path.getsize(path), "bytes")


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else ctypes.util.find_library("cfitsio")
    if not so:
        raise SystemExit("libcfitsio not found: pass its path")
    L = C.CDLL(so)
    out = os.path.join(HERE, "fits")
    os.makedirs(out, exist_ok=True)
    for npix in test_fits.ALL_TYPES_NPIX:
        img, _, _, keys = test_fits.all_types_case(npix)
        path = os.path.join(out, f"all_types_{npix}.fits")
        if os.path.exists(path):
            os.unlink(path)  # ffinit refuses to overwrite
        cfitsio_write(L, path, img, keys)
    path = os.path.join(out, "double_edge_cases.fits")
    if os.path.exists(path):
        os.unlink(path)
    cfitsio_write(L, path, np.zeros((4, 4), np.float32), test_fits.edge_keys())


if __name__ == "__main__":
    main()
