#!/usr/bin/env python3
"""Writes basis_universal_amd/csrc/psnr_hvs_tables.inc: the constants of PSNR-HVS / PSNR-HVS-M as hexadecimal binary32 literals (exact in every compiler, and in
tests/psnr_hvs_helpers.py, which reads this file with float.fromhex).

  HVS_COS[u * 8 + x], HVS_ALPHA[2]   dct2f::init(8, 8) of the reference (transcoder/basisu_transcoder.cpp:26630-26660) in its own binary32 expression order:
        angle = (pi_f * float((2 x + 1) u)) / (2.0f * 8.0f), cos = cosf(angle); alpha[0] = sqrtf(1.0f / 8.0f), alpha[1] = sqrtf(2.0f * (1.0f / 8.0f)).
        cosf and sqrtf are the C library's of the machine this runs on, called through ctypes -- the call the reference build makes there. The product never calls
        cosf: what it multiplies with is this table.
  HVS_CSF[64], HVS_MASK[64]          the published PSNR-HVS-M coefficients (Ponomarenko et al., psnrhvsm.m: CSFCof and MaskCof), six decimals each. Both follow from the
        JPEG luminance quantisation table q (ITU-T T.81, table K.1): MaskCof = (10 / q)^2 and CSFCof = 25.73509 / q (its largest entry, q = 10, is 2.573509),
        rounded to six decimals, then to the nearest binary32 as a compiler reads the decimal literal.
usage: gen_psnr_hvs_tables.py            (rewrites the file; byte-stable wherever cosf rounds alike)"""
import ctypes
import ctypes.util
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "basis_universal_amd" / "csrc" / "psnr_hvs_tables.inc"

JPEG_LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61,
               12, 12, 14, 19, 26, 58, 60, 55,
               14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77,
               24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101,
               72, 92, 95, 98, 112, 100, 103, 99]
CSF_TIMES_Q = 25.73509


def libm():
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (m.cosf, m.sqrtf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return m


def dct_tables():
    f, m = np.float32, libm()
    pi = f(3.14159265358979323846)
    cos = [m.cosf(float(f(pi * f((2 * x + 1) * u)) / f(f(2.0) * f(8.0)))) for u in range(8) for x in range(8)]
    inv = f(1.0) / f(8.0)
    alpha = [m.sqrtf(float(inv)), m.sqrtf(float(f(2.0) * inv))]
    return np.array(cos, np.float32), np.array(alpha, np.float32)


def published(value):
    """six decimals, as the coefficients were published, then the binary32 nearest to that decimal"""
    return np.float32(f"{value:.6f}")


def hvs_tables():
    csf = np.array([published(CSF_TIMES_Q / q) for q in JPEG_LUMA_Q], np.float32)
    mask = np.array([published((10.0 / q) ** 2) for q in JPEG_LUMA_Q], np.float32)
    return csf, mask


def rows(name, values, comment):
    lines = [f"// {comment}", f"BU_HVS_TAB float {name}[{values.size}] = {{"]
    for k in range(0, values.size, 8):
        lines.append("    " + " ".join(f"{float(v).hex()}f," for v in values[k:k + 8]) + "   // " + " ".join(f"{float(v):.9g}" for v in values[k:k + 8]))
    return lines + ["};"]


def text():
    cos, alpha = dct_tables()
    csf, mask = hvs_tables()
    out = ["// psnr_hvs_tables.inc -- written by tools/gen_psnr_hvs_tables.py; do not edit.", "// BU_HVS_TAB is defined by the includer (psnr_hvs.h): `static const` on the host, `static __device__ const` under hipcc.", ""]
    out += rows("HVS_COS", cos, "cos table of the 8-point DCT-II, [frequency * 8 + sample]") + [""]
    out += rows("HVS_ALPHA", alpha, "its scaling: frequency 0, every other frequency") + [""]
    out += rows("HVS_CSF", csf, "contrast sensitivity coefficients, [row * 8 + column] of the DCT block") + [""]
    out += rows("HVS_MASK", mask, "masking coefficients, same order") + [""]
    return "\n".join(out)


if __name__ == "__main__":
    OUT.write_text(text())
    print("wrote", OUT)
