"""Restatement of colour-managed input (TEST INFRASTRUCTURE): the tables cavif_rs_amd/csrc/icc_reader.h specifies, the integer arithmetic
cavif_rs_amd/csrc/dev_colour.h specifies, and a float64 statement of the same transform to judge both against.  It works from a *description* of a source
(curves and colorants as Python numbers), never from profile bytes: tests/helpers/colour_cases.py writes the bytes from the same description.

The tables are made with Python floats (IEEE doubles, one operation per step, math.pow = the C library's pow), in the order icc_reader.h gives, so they equal
the library's integers; tests/test_icc_reader.py checks that they do.  tests/test_colour_reference.py checks this file by hand-worked values and against LCMS2.

A curve is ('identity',), ('gamma', g), ('table', [uint16 ...]) or ('para', ftype, [g, a, b, c, d, e, f][:n]).  Colorants are [[X Y Z of R], [.. G], [.. B]].
"""
import math

import numpy as np

FRAC, MBITS, LIN16_SEG, OUT16_SEG = 24, 30, 4096, 8192
ONE = 1 << FRAC
D50 = (0.9642, 1.0, 0.8249)
SRGB_CHRM = (0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06)
BRADFORD = ((0.8951, 0.2664, -0.1614), (-0.7502, 1.7135, 0.0367), (0.0389, -0.0685, 1.0296))


def s15f16(v):
    """the value an s15Fixed16 field holds for v (what a profile on disk says)"""
    return int(round(v * 65536.0)) / 65536.0


# ------------------------------------------------------------------------------------------------------------------------------------ curves
def curve_eval(curve, x):
    kind = curve[0]
    y = x
    if kind == 'gamma':
        y = math.pow(x, curve[1])
    elif kind == 'table':
        t = curve[1]
        n = len(t)
        pos = x * float(n - 1)
        i = min(int(pos), n - 2)
        f = pos - float(i)
        y = (float(t[i]) + (float(t[i + 1]) - float(t[i])) * f) / 65535.0
    elif kind == 'para':
        ftype, p = curve[1], list(curve[2]) + [0.0] * 7
        g = p[0]
        a, b = (p[1], p[2]) if ftype >= 1 else (1.0, 0.0)
        c = p[3] if ftype >= 2 else 0.0
        d = p[4] if ftype >= 3 else 0.0
        e, f = (p[5], p[6]) if ftype == 4 else (0.0, 0.0)

        def power(t):
            return math.pow(t, g) if t > 0.0 else 0.0
        if ftype == 0:
            y = power(x)
        elif ftype == 1:
            y = power(a * x + b) if a * x + b >= 0.0 else 0.0
        elif ftype == 2:
            y = power(a * x + b) + c if a * x + b >= 0.0 else c
        elif ftype == 3:
            y = power(a * x + b) if x >= d else c * x
        else:
            y = power(a * x + b) + e if x >= d else c * x + f
    if not y >= 0.0:
        y = 0.0
    return min(y, 1.0)


def srgb_eotf(e):
    return e / 12.92 if e <= 0.04045 else math.pow((e + 0.055) / 1.055, 2.4)


def srgb_oetf(l):
    return 12.92 * l if l <= 0.0031308 else 1.055 * math.pow(l, 1.0 / 2.4) - 0.055


# ------------------------------------------------------------------------------------------------------------------------------------ matrices (icc_reader.h's loops)
def mat_mul(a, b):
    o = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += a[i][k] * b[k][j]
            o[i][j] = s
    return o


def mat_inv(m):
    c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1]
    c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2]
    c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0]
    det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02
    o = [[0.0] * 3 for _ in range(3)]
    o[0][0] = c00 / det; o[1][0] = c01 / det; o[2][0] = c02 / det
    o[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; o[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; o[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det
    o[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det; o[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det; o[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det
    return o


def colorants_from_chromaticities(c):
    """(white x y, red x y, green x y, blue x y) -> rows X Y Z by columns R G B, the white point Bradford-adapted to D50"""
    W = [c[0] / c[1], 1.0, (1.0 - c[0] - c[1]) / c[1]]
    P = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        x, y = c[2 + 2 * j], c[3 + 2 * j]
        P[0][j] = x / y; P[1][j] = 1.0; P[2][j] = (1.0 - x - y) / y
    Pi = mat_inv(P)
    S = []
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += Pi[i][k] * W[k]
        S.append(s)
    N = [[P[i][j] * S[j] for j in range(3)] for i in range(3)]
    Bi = mat_inv(BRADFORD)
    cs, cd = [], []
    for i in range(3):
        s, d = 0.0, 0.0
        for k in range(3):
            s += BRADFORD[i][k] * W[k]
            d += BRADFORD[i][k] * D50[k]
        cs.append(s); cd.append(d)
    DB = [[(cd[i] / cs[i]) * BRADFORD[i][j] for j in range(3)] for i in range(3)]
    return mat_mul(mat_mul(Bi, DB), N)


def matrix_double(colorants_xyz_rows):
    """inverse(sRGB colorants, D50) * (source colorants): float64, rows = output channel"""
    return mat_mul(mat_inv(colorants_from_chromaticities(SRGB_CHRM)), colorants_xyz_rows)


def rows_from_columns(cols):
    """[[X Y Z of R], [of G], [of B]] -> rows X, Y, Z by columns R G B"""
    return [[cols[j][i] for j in range(3)] for i in range(3)]


# ------------------------------------------------------------------------------------------------------------------------------------ the baked transform
def q(v):
    if not v >= 0.0:
        v = 0.0
    return int(math.floor(min(v, 1.0) * 16777216.0 + 0.5))


class Transform:
    """the integers of one baked transform and the float64 statement beside them.  curves: three curve descriptions; M: the double matrix (None: identity matrix)"""

    def __init__(self, curves, M=None):
        self.curves = curves
        self.M = M if M is not None else [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        self.matrix = np.array([[int(math.floor(self.M[i][j] * 1073741824.0 + 0.5)) for j in range(3)] for i in range(3)], dtype=np.int64)
        self.lin8 = np.array([[q(curve_eval(c, v / 255.0)) for v in range(256)] for c in curves], dtype=np.int64)
        lin16 = [[q(curve_eval(c, i / float(LIN16_SEG))) for i in range(LIN16_SEG + 1)] for c in curves]
        self.lin16 = np.array([l + [l[-1]] for l in lin16], dtype=np.int64)
        self.U = np.array([0] + [int(math.ceil(16777216.0 * srgb_eotf((2 * k - 1) / 510.0))) for k in range(1, 256)], dtype=np.int64)
        out16 = [int(math.floor(65535.0 * srgb_oetf(i / float(OUT16_SEG)) + 0.5)) for i in range(OUT16_SEG + 1)]
        self.out16 = np.array(out16 + [out16[-1]], dtype=np.int64)

    # -- dev_colour.h, in int64 (numpy's // and >> floor towards minus infinity)
    def _mix(self, x):
        """x: (..., 3) linear values -> (..., 3) clipped linear values"""
        y = np.stack([self.matrix[i, 0] * x[..., 0] + self.matrix[i, 1] * x[..., 1] + self.matrix[i, 2] * x[..., 2] for i in range(3)], axis=-1)
        return np.clip((y + (1 << 29)) >> 30, 0, ONE)

    def level8(self, y):
        """the number of k in 1..255 with U[k] <= y"""
        return np.searchsorted(self.U[1:], np.asarray(y, np.int64), side='right')

    def level16(self, y):
        y = np.asarray(y, np.int64)
        j, g = y >> 11, y & 2047
        return (self.out16[j] * (2048 - g) + self.out16[j + 1] * g + 1024) >> 11

    def convert8(self, px):
        """(..., 3 | 4) uint8 -> the same shape: colour channels converted, alpha as it was"""
        px = np.asarray(px)
        v = px[..., :3].astype(np.int64)
        x = np.stack([self.lin8[c][v[..., c]] for c in range(3)], axis=-1)
        out = px.copy()
        out[..., :3] = self.level8(self._mix(x)).astype(np.uint8)
        return out

    def convert16(self, px):
        px = np.asarray(px)
        s = px[..., :3].astype(np.int64)
        p = s * 4096
        i = p // 65535
        f = p - i * 65535
        x = np.stack([(self.lin16[c][i[..., c]] * (65535 - f[..., c]) + self.lin16[c][i[..., c] + 1] * f[..., c] + 32767) // 65535 for c in range(3)], axis=-1)
        out = px.copy()
        out[..., :3] = self.level16(self._mix(x)).astype(np.uint16)
        return out

    # -- the same transform in float64: exact curves, the double matrix, clipping in linear light, the sRGB curve, rounding half up
    def convert_float(self, px, peak):
        px = np.asarray(px)
        flat = px[..., :3].reshape(-1, 3).astype(np.float64) / peak
        lin = np.empty_like(flat)
        for c in range(3):
            levels, inverse = np.unique(flat[:, c], return_inverse=True)
            lin[:, c] = np.array([curve_eval(self.curves[c], float(v)) for v in levels])[inverse]
        y = np.clip(lin @ np.array(self.M).T, 0.0, 1.0)
        e = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)
        out = px.copy()
        out[..., :3] = np.floor(e * peak + 0.5).reshape(px[..., :3].shape).astype(px.dtype)
        return out


def from_description(curves, colorant_columns):
    """what mi_colour_transform_from_icc bakes for a profile that holds these curves and colorants ([[X Y Z of R], ..]; as stored: s15Fixed16)"""
    return Transform(curves, matrix_double(rows_from_columns([[s15f16(v) for v in col] for col in colorant_columns])))


def from_png(file_gamma, chrm=None):
    """what mi_colour_transform_from_png bakes; None = the identity"""
    if chrm is None and abs(file_gamma * 2.2 - 1.0) < 0.05:
        return None
    curves = [('gamma', 1.0 / file_gamma)] * 3
    return Transform(curves, matrix_double(colorants_from_chromaticities(chrm)) if chrm is not None else None)
