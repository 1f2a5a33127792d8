"""Float64 restatement of the device shading functions (helper module: no tests in here).

Each function below restates, in double precision, one function of adapt_amd/csrc/shading.hpp or volumetric.hpp (the reference
formulas the oracle, oracle/pt_oracle.c, cites line by line), with the same branch structure and the same reference quirks (the
Fresnel-blend pdf of a back-facing half vector is NaN here too).  The tests hold the float32 code of both builds to it
(tests/test_f64_models.py pins it against the reference-run vectors and the oracle; tests/test_gpu_product_functions.py holds the
product build to it).

Conventions
  * Inputs are the float32 values the device reads; every value is computed from them in float64.
  * DECISIONS on input-level quantities (a sign of a dot product of two input vectors, `max|out - in| > eps`) are taken in float32,
    the way both builds and the oracle take them (`dot` is the same IEEE sequence everywhere), so that an exactly-zero or 1e-7
    cosine lands on the device's side of the branch.  Every other comparison is evaluated in float64 and returns its distance to
    the threshold: `margin` is the smallest such distance a row met.  Float32 code may legitimately take the other branch of a
    comparison whose operand is within a few ulp of its threshold; the tests set those rows aside (and count them).
  * Scale S of an output: `scale()` below - |r| plus the first-order response of r to a relative perturbation of 2^-24 of every
    input, i.e. the size of the rounding a float32 evaluation cannot avoid even when each operation is correctly rounded.  For a
    product or a quotient of well-conditioned terms that is ~|r|; for a cancelling sum it is ~ the sum of the magnitudes of the terms.
  * The row functions are scalar; `rows()` maps one over the rows of an array.
"""
import math

import numpy as np

U = 2.0 ** -24
KNIFE = 1e-6              # rows whose margin is below this are within a knife edge of a float32 branch
INV_PI = 1.0 / math.pi
BRDF_EPS = float(np.float32(1e-7))
F32 = np.float32


# ------------------------------------------------------------------ float64 vector algebra on 3-tuples
def v(a):
    return (float(a[0]), float(a[1]), float(a[2]))


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def hmul(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def norm(a):
    return math.sqrt(dot(a, a))


def normalize(a):
    n = norm(a)
    return mul(a, 1.0 / n) if n > 0 else (math.nan, math.nan, math.nan)


def neg(a):
    return (-a[0], -a[1], -a[2])


def splat(s):
    return (s, s, s)


ZERO = (0.0, 0.0, 0.0)
Y = (0.0, 1.0, 0.0)


def dot32(a, b):
    """the device's dot product of two float32 vectors, in float32 (a decision operand)"""
    a, b = F32(a), F32(b)
    return float((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def sub32(a, b):
    return tuple(float(x) for x in (F32(a) - F32(b)))


class Margin:
    """smallest distance to a knife-edge threshold met while evaluating one row"""
    def __init__(self):
        self.m = math.inf
        self.amp = 1.0
        self.amp_mask = None          # outputs the cancellation factor applies to (None: all of them)

    def cancel(self, val, mag):
        """a sum `val` of terms whose magnitudes add up to `mag`: its relative rounding is amplified by mag / |val|"""
        if math.isfinite(val) and math.isfinite(mag) and mag > 0:
            self.amp = max(self.amp, mag / abs(val) if val != 0 else math.inf)
        return val

    def at(self, x, thr):
        if math.isfinite(x):
            self.m = min(self.m, abs(x - thr))
        return x


# ------------------------------------------------------------------ frames (la/cam_transform.py via shading.hpp)
def rotation_between(fixed, target, mg=None):
    """Rodrigues rotation taking `fixed` onto `target`; diag(sign(c)) when |c| >= 1 - 1e-5 (knife edge)"""
    axis = cross(fixed, target)
    c = dot(fixed, target)
    if mg is not None:
        mg.at(abs(c), 1.0 - 1e-5)
    if abs(c) < 1.0 - 1e-5:
        n = normalize(axis)
        k = 1.0 - c
        return ((c + k * n[0] * n[0], k * n[0] * n[1] - axis[2], k * n[0] * n[2] + axis[1]),
                (k * n[1] * n[0] + axis[2], c + k * n[1] * n[1], k * n[1] * n[2] - axis[0]),
                (k * n[2] * n[0] - axis[1], k * n[2] * n[1] + axis[0], c + k * n[2] * n[2]))
    s = (c > 0) - (c < 0)
    return ((s, 0.0, 0.0), (0.0, s, 0.0), (0.0, 0.0, s))


def mat_mul(R, a):
    return (dot(R[0], a), dot(R[1], a), dot(R[2], a))


def localize(anchor, d, mg=None):
    return mat_mul(rotation_between(anchor, Y, mg), d)


def delocalize(anchor, d, mg=None):
    return mat_mul(rotation_between(Y, anchor, mg), d)


def surface_maps_ns(applied, n_g, n_s, t_normal, t_bump):
    """(n_s, margin) after shade_stage.hpp surface_maps: the normal-map texel taken from the +y frame onto n_g (applied & 2), then the
    bump-map texel delocalized around that shading normal (applied & 4).  n_s: the shading normal the vertex arrives with."""
    mg = Margin()
    n = v(n_s)
    if int(applied) & 2:
        n = mat_mul(rotation_between(Y, v(n_g), mg), v(t_normal))
    if int(applied) & 4:
        n = delocalize(n, v(t_bump), mg)
    return np.array(n), mg


def raw_of_local(l, mg=None):
    """(cos_t, sin_t, cos_p, sin_p) of a local direction (+y = normal); the azimuth is (1, 0) while sin_t <= 1e-5 (knife edge)"""
    cos_t = l[1]
    sin_t = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
    cos_p, sin_p = 1.0, 0.0
    if mg is not None:
        mg.at(sin_t, 1e-5)
    if sin_t > 1e-5:
        cos_p, sin_p = l[0] / sin_t, l[2] / sin_t
    return cos_t, sin_t, cos_p, sin_p


def to_raw(d, normal, mg=None):
    return raw_of_local(localize(normal, d, mg), mg)


# ------------------------------------------------------------------ optics (la/geo_optics.py)
def reflect_in(ray, normal):
    return normalize(sub(ray, mul(normal, 2.0 * dot(normal, ray))))


def pow5(x):
    return x ** 5


def schlick(r_s, c):
    p = pow5(1.0 - c)
    return tuple(r + (1.0 - r) * p for r in r_s)


def fresnel_dielectric(n_in, n_out, cos_inc, cos_ref, mg=None):
    a, b, c, d = n_in * cos_inc, n_out * cos_inc, n_in * cos_ref, n_out * cos_ref
    if mg is not None:
        mg.cancel(a - d, abs(a) + abs(d)); mg.cancel(c - b, abs(c) + abs(b))
    rs = (a - d) / (a + d) if a + d != 0 else math.nan
    rp = (c - b) / (c + b) if c + b != 0 else math.nan
    return 0.5 * (rs * rs + rp * rp)


def tir_term(dot_normal, ni, nr):
    """1 - (ni/nr)^2 (1 - cos^2): total reflection where it is < 0 (knife edge at 0)"""
    return 1.0 - (ni / nr) ** 2 * (1.0 - dot_normal * dot_normal)


def refract_snell(incid, normal, dot_n, ni, nr, mg=None):
    exiting = (dot_n > 0) - (dot_n < 0)
    ratio = ni / nr
    cos_r2 = 1.0 - ratio * ratio * (1.0 - dot_n * dot_n)
    if mg is not None:
        mg.cancel(cos_r2, 1.0 + ratio * ratio * (1.0 - dot_n * dot_n))
    if cos_r2 > 0:
        return normalize(add(sub(mul(incid, ratio), mul(normal, ratio * dot_n)), mul(normal, exiting * math.sqrt(cos_r2)))), cos_r2
    return ZERO, cos_r2


def omf(F, mg):
    """1 - F, a cancelling sum where F -> 1"""
    return mg.cancel(1.0 - F, 1.0 + abs(F))


def spow(b, e):
    """the reference's pow on a non-negative base: 0^0 = 1, 0^e = 0 for e > 0"""
    if b == 0.0:
        return 1.0 if e == 0.0 else 0.0
    return b ** e


# ------------------------------------------------------------------ materials
class Mat:
    """one packed material row: int32[4] = (type, is_delta, is_bsdf, 0), float32[13] = k_d, k_s, k_g, mean, ior"""
    def __init__(self, mi, mf):
        self.type, self.is_delta, self.is_bsdf = int(mi[0]), int(mi[1]), int(mi[2])
        f = [float(x) for x in mf]
        self.k_d, self.k_s, self.k_g, self.mean, self.ior = tuple(f[0:3]), tuple(f[3:6]), tuple(f[6:9]), tuple(f[9:12]), f[12]


def lambert_eval(b, n, out):
    c = max(0.0, dot(n, out))
    return mul(b.k_d, INV_PI * c)


def blinn_phong_eval(b, n_s, incid, out):
    c = max(0.0, dot(n_s, out))
    h = sub32(out, incid)
    h = normalize(h) if max(abs(x) for x in h) > BRDF_EPS else ZERO
    dc = max(0.0, dot(h, n_s))
    glossy = tuple(spow(dc, e) for e in b.k_g)
    return tuple((kd + ks * ((kg + 2.0) * 0.5) * g) * INV_PI * c for kd, ks, kg, g in zip(b.k_d, b.k_s, b.k_g, glossy))


def mod_phong_eval(b, n_s, incid, out):
    dn = dot32(n_s, out)
    if not dn > 0:
        return ZERO
    dn = dot(n_s, out)
    refl = normalize(sub(mul(n_s, 2.0 * dn), out))
    dv = max(0.0, -dot(incid, refl))
    spec = tuple(((kg + 2.0) * 0.5) * spow(dv, kg) * ks * INV_PI * dn for kg, ks in zip(b.k_g, b.k_s))
    return add(spec, lambert_eval(b, n_s, out))


def fb_cos2_sin2(h, normal, R, d_half, mg):
    tx = mat_mul(R, (1.0, 0.0, 0.0))
    t = sub(h, mul(normal, d_half))
    if norm(t) > 0:                                   # the azimuth of a half vector along the normal is 0 / 0 (NaN in every build)
        mg.at(norm(t), 0.0)
    d = dot(tx, normalize(t))
    return d * d, 1.0 - d * d


def fresnel_blend_eval(b, n_s, incid, out, R, mg):
    h = sub32(out, incid)
    if not (dot32(n_s, out) > 0 and max(abs(x) for x in h) > float(F32(1e-4))):
        mg.at(max(abs(x) for x in h), 1e-4)
        return ZERO
    mg.at(max(abs(x) for x in h), 1e-4)
    h = normalize(h)
    d_out = dot(n_s, out)
    d_in = -dot(n_s, incid)
    d_half = abs(dot(n_s, h))
    d_hk = abs(dot(h, out))
    F = schlick(b.k_s, d_hk)
    c2, s2 = fb_cos2_sin2(h, n_s, R, d_half, mg)
    denom = d_hk * max(d_in, d_out)
    lobe = b.k_g[2] * spow(d_half, b.k_g[0] * c2 + b.k_g[1] * s2)
    k = 28.0 / (23.0 * math.pi)
    p_in, p_out = pow5(1.0 - d_in / 2.0), pow5(1.0 - d_out / 2.0)
    mg.cancel(1.0 - p_in, 1.0 + p_in); mg.cancel(1.0 - p_out, 1.0 + p_out)
    return tuple((f * lobe / denom + kd * k * (1.0 - ks) * ((1.0 - p_in) * (1.0 - p_out))) * d_out
                 for f, kd, ks in zip(F, b.k_d, b.k_s))


def oren_nayar_eval(b, n_s, incid, out, mg):
    ci, si, cpi, spi = to_raw(neg(incid), n_s, mg)
    co, so, cpo, spo = to_raw(out, n_s, mg)
    max_cos = max(0.0, cpi * cpo + spi * spo) if (si > 1e-5 and so > 1e-5) else 0.0
    aci, aco = abs(ci), abs(co)
    if aci > aco:
        sin_alpha, tan_beta = so, si / aci
    else:
        sin_alpha, tan_beta = si, so / aco if aco > 0 else math.inf
    f = b.k_g[0] + b.k_g[1] * max_cos * sin_alpha * tan_beta
    return mul(b.k_d, INV_PI * f * abs(co))


def thin_coat_eval(b, n_s, incid, out, mg):
    refl = reflect_in(incid, n_s)
    d_in = dot(incid, n_s)
    refra_in, cos_r2 = refract_snell(incid, n_s, d_in, 1.0, b.k_g[2], mg)
    F_in = fresnel_dielectric(1.0, b.k_g[2], abs(d_in), math.sqrt(max(cos_r2, 0.0)) if cos_r2 >= 0 else math.nan, mg)
    if mg.at(abs(dot(out, refl)), 1.0 - 1e-4) > 1.0 - 1e-4:
        return mul(b.k_s, F_in)
    d_out = dot(out, n_s)
    refra_out, cos_r2 = refract_snell(out, n_s, d_out, 1.0, b.k_g[2], mg)
    F_out = fresnel_dielectric(1.0, b.k_g[2], abs(d_out), math.sqrt(cos_r2) if cos_r2 >= 0 else math.nan, mg)
    return mul(oren_nayar_eval(b, n_s, refra_in, refra_out, mg), omf(max(F_in, F_out), mg))


def thin_coat_fresnel(b, n_s, incid, mg):
    d_in = dot(incid, n_s)
    cos_r2 = mg.cancel(1.0 - (1.0 / b.k_g[2]) ** 2 * (1.0 - d_in * d_in), 2.0)
    return fresnel_dielectric(1.0, b.k_g[2], abs(d_in), math.sqrt(cos_r2) if cos_r2 >= 0 else math.nan, mg)


# Trowbridge-Reitz microfacet (type 3): k_g = (alpha_x, alpha_y, .), k_s = (ior outside, ior inside, .)
def fresnel_eval(cos_v, n_in, n_tr, mg):
    neg_ = cos_v < 0
    cv = -cos_v if neg_ else cos_v
    ior_in, ior_tr = (n_tr, n_in) if neg_ else (n_in, n_tr)
    sin_v = math.sqrt(max(0.0, 1.0 - cv * cv))
    sin_t = ior_in / ior_tr * sin_v
    return fresnel_dielectric(ior_in, ior_tr, cv, math.sqrt(max(0.0, 1.0 - sin_t * sin_t)), mg)


def tr_D(raw, ax, ay):
    cos_t, sin_t, cos_p, sin_p = raw
    if not cos_t > 0:
        return 0.0
    d2 = cos_t * cos_t
    e = (cos_p * cos_p / (ax * ax) + sin_p * sin_p / (ay * ay)) * (sin_t * sin_t / d2)
    return 1.0 / (math.pi * ax * ay * d2 * d2 * (1.0 + e) * (1.0 + e))


def tr_lambda(d, ax, ay, normal, mg):
    cos_t, sin_t, cos_p, sin_p = to_raw(d, normal, mg)
    abs_cos = abs(cos_t)
    mg.at(abs_cos, 1e-5)
    if not abs_cos > 1e-5:
        return 0.0
    alpha = math.sqrt(cos_p * cos_p * ax * ax + sin_p * sin_p * ay * ay)
    at2 = (alpha * sin_t / abs_cos) ** 2
    return mg.cancel(-1.0 + math.sqrt(1.0 + at2), 1.0 + math.sqrt(1.0 + at2)) * 0.5


def tr_G1(d, ax, ay, normal, mg):
    return 1.0 / (1.0 + tr_lambda(d, ax, ay, normal, mg))


def tr_G(incid, out, ax, ay, normal, mg):
    return 1.0 / (1.0 + tr_lambda(incid, ax, ay, normal, mg) + tr_lambda(out, ax, ay, normal, mg))


def tr_pdf(incid, wh, ax, ay, normal, mg):
    return tr_D(to_raw(wh, normal, mg), ax, ay) * tr_G1(incid, ax, ay, normal, mg) * abs(dot(wh, incid)) / abs(dot(normal, incid))


def microfacet_eval_raw(b, n_s, wh, raw, incid, out, mg):
    if not max(abs(x) for x in wh) > BRDF_EPS:
        return ZERO
    wh = normalize(wh)
    fres = fresnel_eval(dot(wh, out), b.k_s[0], b.k_s[1], mg)
    k = tr_D(raw, b.k_g[0], b.k_g[1]) * tr_G(neg(incid), out, b.k_g[0], b.k_g[1], n_s, mg) * fres * abs(dot(n_s, out))
    return mul(b.k_d, k)


def microfacet_eval(b, n_s, incid, out, mg):
    cm32 = F32(dot32(n_s, out)) * F32(dot32(n_s, incid))
    if not cm32 < 0:
        return ZERO
    cos_mult = dot(n_s, out) * dot(n_s, incid)
    wh = normalize(sub(out, incid))
    return mul(microfacet_eval_raw(b, n_s, wh, to_raw(wh, n_s, mg), incid, out, mg), 1.0 / (-4.0 * cos_mult))


def brdf_eval(b, n_s, n_g, incid, out, mg):
    if not F32(dot32(incid, n_g)) * F32(dot32(out, n_g)) < 0:
        return ZERO
    t = b.type
    if t == 0:
        return blinn_phong_eval(b, n_s, incid, out)
    if t == 1:
        return lambert_eval(b, n_s, out)
    if t == 4:
        return mod_phong_eval(b, n_s, incid, out)
    if t == 5:
        return fresnel_blend_eval(b, n_s, incid, out, rotation_between(Y, n_s, mg), mg)
    if t == 6:
        return oren_nayar_eval(b, n_s, incid, out, mg)
    if t == 7:
        return thin_coat_eval(b, n_s, incid, out, mg)
    if t == 3:
        return microfacet_eval(b, n_s, incid, out, mg)
    return ZERO


def brdf_pdf(b, n_s, outdir, incid, mg):
    if not F32(dot32(n_s, outdir)) * F32(dot32(n_s, incid)) < 0:
        return 0.0
    d_out = dot(n_s, outdir)
    t = b.type
    if t in (0, 1, 6):
        return d_out * INV_PI
    if t == 4:
        g = b.mean[2]
        dro = max(0.0, dot(reflect_in(incid, n_s), outdir))
        return max(b.k_d) * d_out * INV_PI + max(b.k_s) * 0.5 * (g + 1.0) * INV_PI * spow(dro, g)
    if t == 7:
        F = thin_coat_fresnel(b, n_s, incid, mg)
        a = mg.at(abs(dot(outdir, reflect_in(incid, n_s))), 1.0 - 1e-3)
        return F if a > 1.0 - 1e-3 else omf(F, mg) * d_out * INV_PI
    if t == 5:
        h = normalize(sub(outdir, incid))
        d_half = dot(h, n_s)
        c2, s2 = fb_cos2_sin2(h, n_s, rotation_between(Y, n_s, mg), d_half, mg)
        e = b.k_g[0] * c2 + b.k_g[1] * s2
        hp = b.k_g[2] * (math.nan if d_half < 0 and e != int(e) else (spow(d_half, e) if d_half >= 0 else d_half ** e))
        return 0.5 * (hp / abs(dot(incid, h)) + d_out * INV_PI)
    if t == 3:
        wh = normalize(sub(outdir, incid))
        return tr_pdf(neg(incid), wh, b.k_g[0], b.k_g[1], n_s, mg) / (-4.0 * dot(wh, incid))
    return 0.0


# ------------------------------------------------------------------ BSDFs (bxdf/bsdf.py)
def _sides(d_out, b, world_ior):
    entering = d_out < 0
    return (world_ior, b.ior) if entering else (b.ior, world_ior)


def glass_eval(b, n_s, incid, out, world_ior, mg):
    d_out = dot(out, n_s)
    ni, nr = _sides(dot32(out, n_s), b, world_ior)
    ref_dir = normalize(sub(out, mul(n_s, 2.0 * d_out)))
    t = mg.at(tir_term(d_out, ni, nr), 0.0)
    if t < 0:
        return b.k_d if mg.at(dot(ref_dir, incid), 1.0 - 5e-5) > 1.0 - 5e-5 else ZERO
    refra, cos_r2 = refract_snell(out, n_s, d_out, ni, nr, mg)
    if cos_r2 > 0:
        F = fresnel_dielectric(ni, nr, abs(d_out), math.sqrt(cos_r2), mg)
        if mg.at(dot(refra, incid), 1.0 - 1e-4) > 1.0 - 1e-4:
            return mul(b.k_d, omf(F, mg))
        if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4:
            return mul(b.k_d, F)
        return ZERO
    return b.k_d if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4 else ZERO


def lambert_trans_eval(b, n_s, incid, out, world_ior, mg):
    d_out = dot(out, n_s)
    ni, nr = _sides(dot32(out, n_s), b, world_ior)
    ref_dir = normalize(sub(out, mul(n_s, 2.0 * d_out)))
    if mg.at(tir_term(d_out, ni, nr), 0.0) < 0:
        return b.k_d if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4 else ZERO
    cos_r2 = mg.cancel(tir_term(d_out, ni, nr), 1.0 + (ni / nr) ** 2 * (1.0 - d_out * d_out))
    F = fresnel_dielectric(ni, nr, abs(d_out), math.sqrt(cos_r2), mg)
    if F32(dot32(incid, n_s)) * F32(dot32(out, n_s)) < 0:
        return mul(b.k_d, F) if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4 else ZERO
    return mul(b.k_d, omf(F, mg) * INV_PI * abs(d_out))


def bsdf_pdf(b, n_s, outdir, incid, world_ior, mg):
    d_out = dot(outdir, n_s)
    ni, nr = _sides(dot32(outdir, n_s), b, world_ior)
    ref_dir = normalize(sub(outdir, mul(n_s, 2.0 * d_out)))
    refra, cos_r2 = refract_snell(outdir, n_s, d_out, ni, nr, mg)
    if mg.at(cos_r2, 0.0) > 0:
        F = fresnel_dielectric(ni, nr, abs(d_out), math.sqrt(cos_r2), mg)
        if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4:
            return F
        if b.type == 0 and mg.at(dot(refra, incid), 1.0 - 1e-4) > 1.0 - 1e-4:
            return omf(F, mg)
        if b.type == 1 and F32(dot32(incid, n_s)) * F32(dot32(outdir, n_s)) > 0:
            return omf(F, mg) * abs(d_out) * INV_PI
        return 0.0
    return 1.0 if mg.at(dot(ref_dir, incid), 1.0 - 1e-4) > 1.0 - 1e-4 else 0.0


def surface_eval_pdf(mi, mf, n_s, n_g, incid, out, world_ior):
    """what apt_bxdf_probe's eval mode returns for one row: (e_r, e_g, e_b, pdf), and the row's knife-edge margin"""
    b, mg = Mat(mi, mf), Margin()
    n_s, n_g, incid, out = v(n_s), v(n_g), v(incid), v(out)
    if b.is_bsdf:
        e = (glass_eval if b.type == 0 else lambert_trans_eval)(b, n_s, incid, out, world_ior, mg) if b.type in (0, 1) else ZERO
        p = bsdf_pdf(b, n_s, out, incid, world_ior, mg)
    else:
        e = brdf_eval(b, n_s, n_g, incid, out, mg)
        p = brdf_pdf(b, n_s, out, incid, mg)
    return np.array([*e, p]), mg


# ------------------------------------------------------------------ sampling densities (the sampler's own pdf and spec at the
# direction it returned; `u` = the row's uniform draws, float32 values, which decide the branch the sampler took)
def _rf(word):
    return (int(word) >> 8) * 2.0 ** -24


def cosine_pdf(n, d):
    return dot(n, d) * INV_PI


def sample_density(mi, mf, n_s, n_g, incid, world_ior, d, words):
    """(spec rgb, pdf) the device sampler must return with direction `d`, or None where it returned no sample of a density
    (delta interactions, the absorbed branch of modified Phong is returned with its constant pdf); and the knife-edge margin."""
    b, mg = Mat(mi, mf), Margin()
    n_s, n_g, incid, d = v(n_s), v(n_g), v(incid), v(d)
    u = [_rf(w) for w in words]
    t = b.type
    spec = None
    if b.is_bsdf:
        if t != 1:
            return None, mg
        dn = dot(incid, n_s)
        ni, nr = _sides(dot32(incid, n_s), b, world_ior)
        if mg.at(tir_term(dn, ni, nr), 0.0) < 0:
            return None, mg
        F = fresnel_dielectric(ni, nr, abs(dn), math.sqrt(mg.cancel(tir_term(dn, ni, nr), 2.0)), mg)
        if not mg.at(u[0], F) > F:
            return None, mg
        n = mul(n_s, (dn > 0) - (dn < 0))
        c = dot(n, d)
        return np.array([*mul(b.k_d, INV_PI * max(0.0, c) * omf(F, mg)), c * INV_PI * omf(F, mg)]), mg
    if t in (0, 1, 6):
        pdf = cosine_pdf(n_s, d)
        spec = blinn_phong_eval(b, n_s, incid, d) if t == 0 else lambert_eval(b, n_s, d)
    elif t == 4:
        kd, ks = max(b.k_d), max(b.k_s)
        mg.at(u[0], kd)
        mg.at(u[0], float(F32(kd) + F32(ks)))
        if u[0] < kd:
            pdf, spec = kd * cosine_pdf(n_s, d), lambert_eval(b, n_s, d)
        elif u[0] < float(F32(kd) + F32(ks)):
            h = normalize(sub(d, incid))
            c = dot(h, n_s)
            if c < 0:
                c = -c
            a = b.mean[2]
            pdf, spec = ks * 0.5 * (1.0 + a) * spow(c, a) * INV_PI, mod_phong_eval(b, n_s, incid, d)
        else:
            pdf, spec = 1.0 - kd - ks, ZERO
    elif t == 5:
        nu, nv = b.k_g[0], b.k_g[1]
        e1 = float(F32(u[0]) * F32(4.0))
        inner = e1 - math.floor(e1)
        tan_phi = math.sqrt((nu + 1.0) / (nv + 1.0)) * math.tan(math.pi / 2 * inner)
        cos_phi2 = 1.0 / (1.0 + tan_phi * tan_phi)
        sin_phi2 = 1.0 - cos_phi2
        cos_phi = math.sqrt(cos_phi2) * (-1.0 if 1.0 < e1 <= 3.0 else 1.0)
        sin_phi = math.sqrt(sin_phi2) * ((2.0 > e1) - (2.0 < e1))
        pc = nu * cos_phi2 + nv * sin_phi2
        cos_t = (1.0 - u[1]) ** (1.0 / (pc + 1.0))
        sin_t = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
        R = rotation_between(Y, n_s, mg)
        half = mat_mul(R, (cos_phi * sin_t, cos_t, sin_phi * sin_t))
        d_inc = dot(incid, half)
        out0 = normalize(sub(incid, mul(half, 2.0 * d_inc)))
        pdf = b.k_g[2] * spow(dot(half, n_s), pc) / max(abs(d_inc), BRDF_EPS)
        valid = mg.at(dot(n_s, out0), 0.0) > 0
        mg.at(u[2], 0.5)
        pdf = 0.5 * (pdf + abs(dot(d, n_s)) * INV_PI)
        spec = fresnel_blend_eval(b, n_s, incid, d, R, mg) if valid else ZERO
    elif t == 3:
        half = normalize(sub(d, incid))
        dot_val = -dot(incid, half)
        co, ci = dot(n_s, d), dot(n_s, incid)
        co32, ci32 = dot32(n_s, d), dot32(n_s, incid)    # both are dot products of float32 inputs (d is the returned direction)
        if not (mg.at(dot_val, 0.0) > 0 and F32(co32) * F32(ci32) < 0 and min(abs(co32), abs(ci32)) > BRDF_EPS):
            return None, mg
        ax, ay = b.k_g[0], b.k_g[1]
        spec = mul(microfacet_eval_raw(b, n_s, half, to_raw(half, n_s, mg), incid, d, mg), 1.0 / (4.0 * abs(co) * abs(ci)))
        pdf = tr_pdf(neg(incid), half, ax, ay, n_s, mg) / (4.0 * dot_val)
    elif t == 7:
        dn = dot(incid, n_s)
        _, cr2 = refract_snell(incid, n_s, dn, 1.0, b.k_g[2], mg)
        refra_in, _ = refract_snell(incid, n_s, dn, 1.0, b.k_g[2], mg)
        F_in = fresnel_dielectric(1.0, b.k_g[0], abs(dn), math.sqrt(cr2) if cr2 >= 0 else math.nan, mg)
        if not mg.at(u[0], F_in) > F_in:
            return None, mg
        # the cosine-hemisphere direction the draws made, then refracted out of the coat (or kept, under total reflection)
        ct, st = math.sqrt(u[1]), math.sqrt(1.0 - u[1])
        phi = float(F32(2.0 * math.pi) * F32(u[2]))
        out0 = delocalize(n_s, (math.cos(phi) * st, ct, math.sin(phi) * st), mg)
        d_out = dot(out0, n_s)
        if mg.at(tir_term(d_out, b.k_g[2], 1.0), 0.0) < 0:
            return np.array([0.0, 0.0, 0.0, ct * INV_PI]), mg
        _, cr2o = refract_snell(out0, n_s, d_out, b.k_g[2], 1.0, mg)
        F_out = fresnel_dielectric(b.k_g[2], 1.0, abs(d_out), math.sqrt(cr2o), mg)
        # density and spec at the RETURNED direction: undo the refraction of d (tangential part / ratio)
        dd = dot(d, n_s)
        tan = sub(d, mul(n_s, dd))
        t0 = mul(tan, 1.0 / b.k_g[2])
        o0 = add(t0, mul(n_s, math.sqrt(max(0.0, 1.0 - dot(t0, t0)))))
        pdf = dot(o0, n_s) * INV_PI * omf(F_in, mg)
        spec = mul(oren_nayar_eval(b, n_s, refra_in, d, mg), omf(F_in, mg) * omf(F_out, mg))
    else:
        return None, mg
    if not dot32(d, n_g) > 0:
        spec = ZERO
    return np.array([*spec, pdf]), mg


def sample_density_row(mi, mf, n_s, n_g, incid, world_ior, d, words):
    """sample_density for reference(): rows without a density come back as NaN with margin -1 (never kept)"""
    y, mg = sample_density(mi, mf, n_s, n_g, incid, world_ior, d, words)
    if y is None:
        mg.m = -1.0
        return np.full(4, np.nan), mg
    return y, mg


# ------------------------------------------------------------------ media (bxdf/phase.py, bxdf/medium.py)
def phase_hg(c, g, mg=None):
    g2 = g * g
    denom = (1.0 + g2) - 2.0 * g * c
    if mg is not None:
        mg.cancel(1.0 - g2, 1.0 + g2); mg.cancel(denom, 1.0 + g2 + abs(2.0 * g * c))
    return (1.0 - g2) / (math.sqrt(denom) * denom) * 0.5 / (2.0 * math.pi)


def phase_rayleigh(c):
    return 0.375 / (2.0 * math.pi) * (1.0 + c * c)


def phase_eval(med_type, mf, c, mg=None):
    par, pdf = mf[10:13], mf[13:16]
    if med_type == 0:
        return phase_hg(c, par[0], mg)
    if med_type == 1:
        p = phase_hg(c, par[0], mg) * pdf[0] + phase_hg(c, par[1], mg) * pdf[1]
        if mg is not None:
            mg.at(pdf[1], 1e-4)
        if pdf[1] > float(F32(1e-4)):
            p += phase_hg(c, par[2], mg) * pdf[2]
        return p
    if med_type == 2:
        return phase_rayleigh(c)
    return 1.0


def medium_eval(med_type, mf, in7):
    """apt_medium_probe mode 2: (phase value, transmittance rgb); in7 = ray_in, ray_out, distance"""
    mf = [float(x) for x in mf]
    mg = Margin()
    c = -dot(v(in7[0:3]), v(in7[3:6]))
    p = phase_eval(med_type, mf, c, mg) if med_type >= 0 else 1.0
    d = float(in7[6])
    return np.array([p] + [math.exp(-mf[7 + k] * d) for k in range(3)]), mg


def medium_scatter_density(med_type, mf, incid, d, words):
    """apt_medium_probe mode 1: the phase value the sampler must return with direction d (the cosine is incid . d)"""
    mf = [float(x) for x in mf]
    mg = Margin()
    if med_type < 0:
        return np.array([1.0]), mg
    c = dot(v(incid), v(d))
    if med_type == 1:
        e = _rf(words[0])
        p0, p1 = mf[13], mf[14]
        mg.at(e, p0); mg.at(e, float(F32(p0) + F32(p1)))
        g = mf[10] if e < p0 else (mf[11] if e < float(F32(p0) + F32(p1)) else mf[12])
        return np.array([phase_hg(c, g, mg)]), mg
    return np.array([phase_eval(med_type, mf, c, mg)]), mg


def medium_mfp(med_type, mf, max_depth, words):
    """apt_medium_probe mode 0 from its draws: (is_mi, t, beta rgb) and the margin of `t >= max_depth`"""
    mf = [float(x) for x in mf]
    mg = Margin()
    ue = mf[7:10]
    idx = int(np.int32(np.uint32(words[0]))) % 3      # pymod: Python's modulo of the raw word read as int32
    rue = max(ue[int(idx)], float(F32(1e-5)))
    t = -math.log(1.0 - _rf(words[1])) / rue
    md = float(max_depth)
    mg.at(t / md if md > 0 else t, 1.0)
    if t >= md:
        tr = [math.exp(-x * md) for x in ue]
        p = sum(tr) / 3.0
        p = p if p > 0 else 1.0
        return np.array([0.0, md] + [x / p for x in tr]), mg
    tr = [math.exp(-x * t) for x in ue]
    p = sum(a * b for a, b in zip(ue, tr)) / 3.0
    p = p if p > 0 else 1.0
    return np.array([1.0, t] + [x * s / p for x, s in zip(tr, mf[1:4])]), mg


# ------------------------------------------------------------------ grid volume (bxdf/volume.py:268-463 via volumetric.hpp vol_*)
# Every decision of the grid-volume functions reports its distance to the branch in units of the float32 error of its operand, derived
# from the operations on the chain (each rounding <= U relative; device logf and glibc logf within 2 U of the true logarithm): Margin.m
# is the smallest such ratio a row met.  A float32 evaluation can take the other branch only where the ratio is below 1; the tests keep
# rows above VOLUME_SAFE = 2 (the second unit is for the model's own operands, which are the float32 inputs taken exactly, against
# intermediate values the float32 code has already rounded).
VOLUME_SAFE = 2.0


def _at_err(mg, x, thr, err):
    """distance of x to thr in units of err (the float32 error bound of x - thr); an exact comparison (err = 0) has no knife edge"""
    if math.isfinite(x) and math.isfinite(thr) and err > 0:
        mg.m = min(mg.m, abs(x - thr) / err)


def _nan_max(a):
    return math.nan if any(math.isnan(x) for x in a) else max(a)


def _nan_min(a):
    return math.nan if any(math.isnan(x) for x in a) else min(a)


def _fmax(a, b):                       # fmaxf / fminf: the non-NaN operand
    return b if math.isnan(a) else (a if math.isnan(b) else max(a, b))


def _fmin(a, b):
    return b if math.isnan(a) else (a if math.isnan(b) else min(a, b))


def volume_intersect(vf, row, mg=None):
    """vol_intersect: (hit, near_t, far_t) and (float32 error bound of near_t, of far_t).  1 / d is +-inf for a zero component; an
    origin on a face plane then gives 0 * inf = NaN for that face, which the element-wise min / max of the two slab distances drops: the
    axis contributes the other face's +-inf to BOTH near and far, and the ray misses (upstream's behaviour, pinned by the fixture).
    Vector.max() / .min() propagate a NaN that survives (both faces NaN), fmaxf / fminf with 0 / max_t drop it."""
    vf = [float(x) for x in vf]
    o, d, max_t = [float(x) for x in row[0:3]], [float(x) for x in row[3:6]], float(row[9])
    lo_t, hi_t = [], []
    for a in range(3):
        inv = math.copysign(math.inf, d[a]) if d[a] == 0 else 1.0 / d[a]
        t1 = (vf[15 + a] - o[a]) * inv if not (vf[15 + a] - o[a] == 0 and math.isinf(inv)) else math.nan
        t2 = (vf[18 + a] - o[a]) * inv if not (vf[18 + a] - o[a] == 0 and math.isinf(inv)) else math.nan
        lo_t.append(_fmin(t1, t2)); hi_t.append(_fmax(t1, t2))       # ti.min / ti.max of two vectors: element-wise fminf / fmaxf, which drop a NaN
    near = _fmax(0.0, _nan_max(lo_t)) + float(F32(1e-5))
    far = _fmin(max_t, _nan_min(hi_t)) - float(F32(1e-5))
    # chain of a slab distance: subtraction, reciprocal, product (3 roundings, the subtraction's relative to its operands), then + 1e-5
    mag = max(abs(o[a]) + max(abs(vf[15 + a]), abs(vf[18 + a])) for a in range(3))
    slope = max((1.0 / abs(d[a]) if d[a] != 0 else 0.0) for a in range(3))
    e_near = U * (mag * slope + 3.0 * abs(near)) if math.isfinite(near) else 0.0
    e_far = U * (mag * slope + 3.0 * abs(far)) if math.isfinite(far) else 0.0
    if mg is not None:
        _at_err(mg, near, far, e_near + e_far)
        _at_err(mg, far, 0.0, e_far)
    hit = bool(near < far and far > 0.0)
    return hit, near, far, e_near, e_far


def volume_density(vi, grid, index, u, ch, mg=None, e_index=(0.0, 0.0, 0.0)):
    """vol_density: the voxel floor(index + (u - 0.5)) of channel ch, 0 outside the grid.  u - 0.5 is exact in float32; the sum rounds
    once (U |index|) on top of the index's own error e_index."""
    res = (int(vi[1]), int(vi[2]), int(vi[3]))
    cell = []
    for a in range(3):
        x = float(index[a]) + (float(u[a]) - 0.5)
        if mg is not None:
            _at_err(mg, x, round(x), e_index[a] + U * (abs(float(index[a])) + 0.5))
        cell.append(math.floor(x))
    if all(0 <= cell[a] < res[a] for a in range(3)):
        return float(grid[cell[2], cell[1], cell[0], ch])
    return 0.0


def _volume_setup(vf, row, words, mg):
    """the part sample_mfp and transmittance share: intersection, local ray, channel pick.  -> None (no hit) or a dict"""
    vf = [float(x) for x in vf]
    hit, near, far, e_near, e_far = volume_intersect(vf, row, mg)
    if not hit:
        return None
    o, d, thp = [float(x) for x in row[0:3]], [float(x) for x in row[3:6]], [float(x) for x in row[6:9]]
    rel = [o[a] - vf[12 + a] for a in range(3)]
    ol = [sum(vf[3 + 3 * i + j] * rel[j] for j in range(3)) for i in range(3)]
    dl = [sum(vf[3 + 3 * i + j] * d[j] for j in range(3)) for i in range(3)]
    # local ray: one subtraction (relative to its operands), three products and two sums per component
    e_ol = [U * sum(abs(vf[3 + 3 * i + j]) * (4.0 * abs(rel[j]) + abs(o[j]) + abs(vf[12 + j])) for j in range(3)) for i in range(3)]
    e_dl = [U * 3.0 * sum(abs(vf[3 + 3 * i + j] * d[j]) for j in range(3)) for i in range(3)]
    pdfs = [thp[c] * vf[24 + c] for c in range(3)]
    tot = (pdfs[0] + pdfs[1]) + pdfs[2]
    pdfs = [p / tot if tot != 0 else math.nan for p in pdfs]
    val = _rf(words[0])
    if math.isnan(pdfs[0]):
        ch = 2                                           # every comparison with NaN is false (all-zero throughput)
    else:
        _at_err(mg, val, pdfs[0], 4.0 * U * pdfs[0]); _at_err(mg, val, pdfs[0] + pdfs[1], 5.0 * U * (pdfs[0] + pdfs[1]))
        ch = 0 if val <= pdfs[0] else (1 if val <= pdfs[0] + pdfs[1] else 2)
    return dict(vf=vf, near=near, far=far, e_near=e_near, e_far=e_far, ol=ol, dl=dl, e_ol=e_ol, e_dl=e_dl, ch=ch, pdf=pdfs[ch],
                inv_maj=1.0 / vf[21 + ch])


def _volume_step(st, t, e_t, word):
    """t -= logf(1 - xi) * inv_maj: the new t and its error bound (logf 2 U, the reciprocal majorant and the product 1.5 U, the sum U |t|)"""
    step = -math.log(1.0 - _rf(word)) * st["inv_maj"]
    t = t + step
    return t, e_t + U * (3.5 * step + abs(t))


def _volume_lookup(st, vi, grid, t, e_t, words3, mg):
    idx = [st["ol"][a] + st["dl"][a] * t for a in range(3)]
    e_idx = [st["e_ol"][a] + st["e_dl"][a] * abs(t) + abs(st["dl"][a]) * e_t + U * (abs(st["ol"][a]) + 2.0 * abs(st["dl"][a] * t)) for a in range(3)]
    return volume_density(vi, grid, idx, [_rf(w) for w in words3], st["ch"], mg, e_idx)


def volume_sample_mfp(vi, vf, grid, row, words):
    """apt_volume_probe mode 2 from its draws: (hit_t, beta rgb, draws) and the margin of every decision.  `words` is a callable
    k -> the k-th 32-bit word of the row's Philox stream."""
    mg = Margin()
    st = _volume_setup(vf, row, [words(0)], mg)
    if st is None:
        return np.array([-1.0, 1.0, 1.0, 1.0, 0.0]), mg
    k = 1
    t, e_t = _volume_step(st, st["near"], st["e_near"], words(k)); k += 1
    Tr, hit_t = 1.0, -1.0
    while True:
        _at_err(mg, t, st["far"], e_t + st["e_far"])
        if not t < st["far"]:
            break
        n_t = _volume_lookup(st, vi, grid, t, e_t, [words(k), words(k + 1), words(k + 2)], mg); k += 3
        p = n_t * st["inv_maj"]
        xi = _rf(words(k)); k += 1
        _at_err(mg, xi, p, 1.5 * U * p)
        if xi < p:
            Tr *= st["vf"][st["ch"]]; hit_t = t
            break
        t, e_t = _volume_step(st, t, e_t, words(k)); k += 1
    beta = [0.0, 0.0, 0.0]
    beta[st["ch"]] = Tr / st["pdf"]
    return np.array([hit_t] + beta + [float(k)]), mg


def volume_transmittance(vi, vf, grid, row, words):
    """apt_volume_probe mode 3 from its draws: (transmittance rgb, draws) and the margin of every decision"""
    mg = Margin()
    st = _volume_setup(vf, row, [words(0)], mg)
    if st is None:
        return np.array([1.0, 1.0, 1.0, 0.0]), mg
    k = 1
    Tr, e_tr, t, e_t = 1.0, 0.0, st["near"], st["e_near"]
    while True:
        t, e_t = _volume_step(st, t, e_t, words(k)); k += 1
        _at_err(mg, t, st["far"], e_t + st["e_far"])
        if t >= st["far"]:
            break
        n_t = _volume_lookup(st, vi, grid, t, e_t, [words(k), words(k + 1), words(k + 2)], mg); k += 3
        f = max(0.0, 1.0 - n_t * st["inv_maj"])
        Tr, e_tr = Tr * f, e_tr * f + U * Tr * (1.5 * n_t * st["inv_maj"] + 1.0 + f)      # the factor's roundings (reciprocal, product, 1 - x) and the product's
        _at_err(mg, Tr, float(F32(0.1)), e_tr)
        if Tr < float(F32(0.1)):
            xi = _rf(words(k)); k += 1
            _at_err(mg, xi, Tr, e_tr)
            if xi >= Tr:
                Tr = 0.0
                break
            Tr, e_tr = 1.0, 0.0
    out = [0.0, 0.0, 0.0]
    out[st["ch"]] = Tr / st["pdf"]
    return np.array(out + [float(k)]), mg


# ------------------------------------------------------------------ emitters (emitters/abtract_source.py)
def emitter_eval_le(src_type, intensity, inci_dir, normal):
    """(le rgb, margin): an area light's radiance toward a ray that arrives at its front side"""
    mg = Margin()
    c = -dot(normalize(v(inci_dir)), v(normal))
    mg.at(c, 0.0)
    return (np.array(v(intensity)) if (src_type == 1 and c > 0) else np.zeros(3)), mg


def emitter_solid_angle_pdf(src_type, inv_area, ray_d, normal, min_depth):
    d = abs(dot(v(ray_d), v(normal)))
    a = float(inv_area) if src_type == 1 else 0.0
    return np.array([a * float(min_depth) ** 2 / d if d > 0 else 0.0]), Margin()


INV_4PI = 0.25 / math.pi
EMITTER_TYPES = {0: "point", 1: "area", 2: "spot", 4: "collimated"}
EMITTER_DRAWS = {"point": 0, "mesh": 3, "sphere": 2, "spot": 0, "collimated": 0}


def emitter_geom(scene, k):
    """what sample_hit reads of the object emitter k is attached to, as the float32 values the device holds: None (no object),
    ("sphere", centre, radius) or ("mesh", dv1, dv2, v0, normals) with dv = the precomputed float32 edge vectors"""
    if int(scene.src_i[k][0]) != 1:
        return None
    first, count, kind = (int(x) for x in scene.obj_info[int(scene.src_i[k][2])])
    P = np.asarray(scene.prims, np.float32).reshape(-1, 3, 3)
    if kind:
        return ("sphere", P[first, 0].copy(), float(P[first, 1, 0]))
    T = P[first:first + count]
    return ("mesh", T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], T[:, 0].copy(), np.asarray(scene.normals, np.float32).reshape(-1, 3)[first:first + count].copy())


def emitter_kind(src_type, geom):
    return geom[0] if int(src_type) == 1 else EMITTER_TYPES[int(src_type)]


def _at_f32(mg, x, thr, err):
    """a decision on a float32 operand whose error bound is `err`: the row is within a knife edge where the operand is within KNIFE of
    the threshold or within four error bounds of it"""
    if math.isfinite(x):
        d = abs(x - thr)
        mg.m = min(mg.m, d, d * KNIFE / (4.0 * err) if err > 0 else math.inf)
    return x


def sample_on_triangle(dv1, dv2, u1, u2, mg=None, fold=None):
    """(point relative to v0, barycentrics of dv1 and dv2 after the fold); the fold is decided on the float32 sum, as every build does"""
    if mg is not None:
        mg.at(u1 + u2, 1.0)
    if (float(F32(u1) + F32(u2)) > 1.0) if fold is None else fold:
        u1, u2 = 1.0 - u1, 1.0 - u2
    return add(mul(dv1, u1), mul(dv2, u2)), (u1, u2)


def uniform_sphere_local(u0, u1, mg=None):
    """sample_uniform_sphere: +y is the pole; phi is the float32 product 2 pi u every build forms"""
    cos_t = 2.0 * u0 - 1.0
    s2 = 1.0 - cos_t * cos_t
    if mg is not None:
        mg.cancel(s2, 1.0 + cos_t * cos_t)
    sin_t = math.sqrt(max(s2, 0.0))
    phi = float(F32(2.0 * math.pi) * F32(u1))
    return (math.cos(phi) * sin_t, cos_t, math.sin(phi) * sin_t)


def emitter_sample_hit(src_type, src_f, geom, hit_pos, words, dn=ZERO, force=None):
    """emitter_sample_hit (shading.hpp; emitters/abtract_source.py:81-158) -> ((pos xyz, intensity rgb, pdf, draws), Margin).
    `words`: the row's Philox words; `dn`: an absolute perturbation of the direction a sphere light constructs (reference()'s
    dir_cols); `force`: {decision: bool} takes the named branch whatever the operands say (the rows placed on an edge, where float32
    decides either way): "dl" (facing away), "pdf" (pdf > 0), "cone", "proj", "rim", "fold", "n2", "depth"."""
    mg = Margin()
    mg.amp_mask = np.array([0, 0, 0, 1, 1, 1, 1, 0], bool)       # hit - pos cancels in the intensity and the pdf, not in the position
    f = [float(x) for x in src_f]
    inten, direc, pos, inv_area, rad = tuple(f[0:3]), tuple(f[3:6]), tuple(f[6:9]), f[9], f[10]
    hit = v(hit_pos)
    t = int(src_type)
    pdf, draws = 1.0, 0
    force = force or {}
    dec = lambda name, cond: force.get(name, cond)
    eps5 = float(F32(1e-5))
    if t == 0:
        x = sub(hit, pos)
        mg.cancel(norm(x), norm(hit) + norm(pos))
        n2 = mg.at(dot(x, x), eps5)
        att = 1.0 / (n2 if dec("n2", n2 > eps5) else eps5)
        mg.at(att, 1.0)
        inten = mul(inten, min(att, 1.0))
    elif t == 1:
        pdf = inv_area
        if geom[0] == "sphere":
            centre, radius = v(geom[1]), geom[2]
            to_hit = normalize(sub(hit, centre))
            local = uniform_sphere_local(_rf(words[0]), _rf(words[1]), mg)
            normal = add(delocalize(to_hit, local, mg), v(dn))
            pos = add(centre, mul(normal, radius))
            pdf = INV_4PI / (radius * radius)
            draws = 2
            e_pos = [U * (abs(centre[a]) + 2.0 * abs(pos[a])) + 4.0 * U * abs(radius) for a in range(3)]
            e_n = 4.0 * U
        else:
            dv1, dv2, v0, normals = geom[1:]
            tri = int(np.int32(np.uint32(words[0]))) % len(dv1)          # pymod of the raw word read as int32
            a1, a2 = v(dv1[tri]), v(dv2[tri])
            pt, (b1, b2) = sample_on_triangle(a1, a2, _rf(words[1]), _rf(words[2]), mg, force.get("fold"))
            pos = add(pt, v(v0[tri]))
            normal = v(normals[tri])
            draws = 3
            # rounding of the point: two products and a sum, the fold's two sums, then + v0 (exact where the point's component is 0)
            e_pos = [U * (3.0 * (abs(a1[a]) + abs(a2[a])) + (abs(pos[a]) if pt[a] != 0.0 else 0.0)) for a in range(3)]
            e_n = 0.0
        diff = sub(hit, pos)
        nd = norm(diff)
        mg.cancel(nd, norm(hit) + norm(pos))
        dl = dot(normalize(diff), normal)
        # float32 error of dl: the position's rounding and the subtraction's through the normal, the direction's own, the dot product's
        e_dl = (sum(abs(normal[a]) * (e_pos[a] + U * abs(diff[a])) for a in range(3)) / nd + e_n + 4.0 * U * abs(dl)) if nd > 0 else 0.0
        _at_f32(mg, dl, 0.0, e_dl)
        if dec("dl", dl <= 0.0):
            inten, pdf = ZERO, 1.0
        else:
            pdf = pdf * (nd * nd / dl) if dl != 0 else math.inf
            inten = mul(inten, 1.0 / pdf) if dec("pdf", pdf > 0.0) and pdf != 0 else ZERO
    elif t == 2:
        th = sub(hit, pos)
        mg.cancel(norm(th), norm(hit) + norm(pos))
        depth = mg.at(norm(th), eps5)
        depth = depth if dec("depth", depth > eps5) else eps5
        cos_v = dot(mul(th, 1.0 / depth), direc)
        mg.at(cos_v, rad)
        inten = mul(inten, 1.0 / (depth * depth)) if dec("cone", cos_v > rad) else ZERO
    elif t == 4:
        pdf = 0.0
        if rad > 0.0:
            th = sub(hit, pos)
            proj = dot(th, direc)
            _at_f32(mg, proj, 0.0, 4.0 * U * sum(abs(th[a] * direc[a]) for a in range(3)))       # hit and pos are inputs: the products and sums round
            if dec("proj", proj > 0.0):
                d2 = mg.cancel(dot(th, th) - proj * proj, dot(th, th) + proj * proj)
                dist = math.sqrt(d2) if d2 >= 0 else math.nan
                # float32 error of dist: the two squares' roundings over 2 dist
                _at_f32(mg, dist, rad, 4.0 * U * (dot(th, th) + proj * proj) / (2.0 * dist) if dist > 0 else math.inf)
                if dec("rim", dist < rad):
                    pos = sub(hit, mul(direc, proj))
                else:
                    inten = ZERO
        else:
            inten = ZERO
    return np.array([*pos, *inten, pdf, float(draws)]), mg

# ------------------------------------------------------------------ conditioning
def reference(fn, cols, float_cols, trials=4, seed=0, dir_cols=(), dir_eps=4 * U):
    """Run a row function over the rows of `cols` -> r (n, k), S (n, k), margin (n,).
    S = max(|r| x the row's cancellation factor, |r| + max over `trials` relative perturbations of +-2^-24 of every float input
    (the columns `float_cols`; the columns `dir_cols`, directions a sampler constructed, take an absolute perturbation of dir_eps per
    component: the few roundings of the sincos / square roots / rotation that made them) of |r' - r| / 2^-24).  A perturbation that crosses a branch makes S large there: such rows are
    also within a knife-edge margin, which the tests count separately."""
    rs = np.random.RandomState(seed)
    R, S, M = [], [], []
    for k in range(len(cols[0])):
        args = [c[k] for c in cols]
        y, mg = fn(*args)
        r = np.asarray(y, np.float64)
        s = np.abs(r)
        for _ in range(trials):
            a = list(args)
            for i in float_cols:
                x = np.asarray(a[i], np.float64)
                a[i] = x * (1.0 + U * rs.choice([-1.0, 1.0], size=x.shape))
            for i in dir_cols:                        # a constructed unit direction: an absolute error of dir_eps per component
                x = np.asarray(a[i], np.float64)
                a[i] = x + dir_eps * rs.choice([-1.0, 1.0], size=x.shape)
            with np.errstate(invalid="ignore"):
                dlt = np.abs(np.asarray(fn(*a)[0], np.float64) - r) / U
            s = np.maximum(s, np.where(np.isnan(r), 0.0, np.where(np.isfinite(dlt), dlt, np.inf)))
        with np.errstate(invalid="ignore"):
            s = np.maximum(s, np.nan_to_num(np.abs(r) * (mg.amp if mg.amp_mask is None else np.where(mg.amp_mask, mg.amp, 1.0)), nan=0.0))
        R.append(r); S.append(s); M.append(mg.m)
    return np.array(R), np.array(S), np.array(M)


# ------------------------------------------------------------------ the input sweep
def _unit(rs, n):
    d = rs.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _frame(nrm):
    t = np.where(np.abs(nrm[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 0, 1.0]]))
    a = np.cross(nrm, t); a /= np.linalg.norm(a, axis=1, keepdims=True)
    return a, np.cross(nrm, a)


def _dir_at_cos(rs, nrm, c):
    """unit directions at cosine c (array) to the normals nrm, random azimuth"""
    a, b = _frame(nrm)
    phi = rs.uniform(0, 2 * np.pi, len(c))
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None]
    return c[:, None] * nrm + s * (np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b)


def _tilt(rs, nrm, max_deg):
    return _dir_at_cos(rs, nrm, np.cos(np.radians(rs.uniform(0, max_deg, len(nrm)))))


def _f32n(x):
    x = np.float32(x)
    return x / np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True).astype(np.float32)


def mat_row(t, k_d, k_s=(0, 0, 0), k_g=(1, 1, 1), is_bsdf=0, is_delta=0, ior=1.0, mean_z=None):
    k_d, k_s, k_g = np.float32(k_d), np.float32(k_s), np.float32(k_g)
    mean = np.float32([k_d.mean(), k_s.mean(), k_g.mean() if mean_z is None else mean_z])
    return np.int32([t, is_delta, is_bsdf, 0]), np.concatenate([k_d, k_s, k_g, mean, [ior]]).astype(np.float32)


def _on(sigma):
    s2 = sigma * sigma
    return 1.0 - s2 / (2.0 * (s2 + 0.33)), 0.45 * s2 / (s2 + 0.09)


GLOSSY = (0.0, 0.5, 1.0, 1e2, 1e3, 1e4)


def _materials(rs):
    """(name, mi, mf, world iors) per material of the sweep: every model and the parameter strata of each"""
    M = []
    kd = lambda: rs.uniform(0.05, 0.95, 3)
    for e in GLOSSY:
        M.append((f"blinn_phong_e{e:g}", *mat_row(0, kd(), rs.uniform(0.05, 0.9, 3), (e, e, e))))
        M.append((f"mod_phong_e{e:g}", *mat_row(4, rs.uniform(0.05, 0.45, 3), rs.uniform(0.05, 0.45, 3), (e, e, e))))
    M.append(("blinn_phong_rgb", *mat_row(0, kd(), rs.uniform(0.05, 0.9, 3), (0.5, 1e2, 1e3))))
    M.append(("mod_phong_rgb", *mat_row(4, rs.uniform(0.05, 0.45, 3), rs.uniform(0.05, 0.45, 3), (1.0, 30.0, 1e3), mean_z=30.0)))
    M.append(("lambertian", *mat_row(1, kd())))
    M.append(("mirror", *mat_row(2, kd(), is_delta=1)))
    for nu, nv in ((10.0, 10.0), (10.0, 1e3), (1e2, 1.0)):
        norm = math.sqrt((nu + 1) * (nv + 1)) / (8 * math.pi)
        M.append((f"fresnel_blend_{nu:g}_{nv:g}", *mat_row(5, kd(), rs.uniform(0.05, 0.5, 3), (nu, nv, norm))))
    for ax, ay in ((1e-3, 1e-3), (0.05, 0.05), (0.5, 0.5), (1.0, 1.0), (0.05, 0.5), (1e-3, 0.5)):
        M.append((f"microfacet_{ax:g}_{ay:g}", *mat_row(3, kd(), (1.0, 1.5, 0.0), (ax, ay, 0.0))))
    for sg in (0.0, 1.5):
        A, B = _on(sg)
        M.append((f"oren_nayar_s{sg:g}", *mat_row(6, kd(), (0, 0, 0), (A, B, sg))))
        M.append((f"thin_coat_s{sg:g}", *mat_row(7, kd(), rs.uniform(0.3, 1.0, 3), (A, B, 1.5))))
    for ior in (1.0001, 1.5, 2.4):
        M.append((f"glass_ior{ior:g}", *mat_row(0, kd(), is_bsdf=1, is_delta=1, ior=ior)))
        M.append((f"lambert_trans_ior{ior:g}", *mat_row(1, kd(), is_bsdf=1, ior=ior)))
    return M


def sweep(seed=0, n_bulk=96, n_edge=32):
    """Deterministic surface-model inputs shared by the CPU and GPU tests.  Columns: mi (n,4) int32, mf (n,13) float32, dirs (n,12)
    float32 = n_s, n_g, incid, out; world_ior (n,) float32; material, stratum (n,) str.  Every material gets a uniform bulk and the
    edge strata below; BSDFs run under world ior 1.0 and 1.33."""
    rs = np.random.RandomState(seed)
    rows_ = {k: [] for k in ("mi", "mf", "dirs", "world_ior", "material", "stratum")}

    def put(name, mi, mf, wior, stratum, n_s, n_g, wi, wo):
        n = len(n_s)
        rows_["mi"].append(np.repeat(mi[None], n, 0)); rows_["mf"].append(np.repeat(mf[None], n, 0))
        rows_["dirs"].append(np.concatenate([_f32n(n_s), _f32n(n_g), _f32n(wi), _f32n(wo)], axis=1).astype(np.float32))
        rows_["world_ior"].append(np.full(n, wior, np.float32))
        rows_["material"].append(np.full(n, name, object)); rows_["stratum"].append(np.full(n, stratum, object))

    for name, mi, mf in _materials(rs):
        bsdf = bool(mi[2])
        for wior in ((1.0, 1.33) if bsdf else (1.0,)):
            nb, ne = n_bulk, n_edge
            # bulk: random normal, shading normal within 30 deg, incid from the upper side, out anywhere
            n_g = _unit(rs, nb); n_s = _tilt(rs, n_g, 30)
            wi = -_dir_at_cos(rs, n_g, rs.uniform(0.02, 1, nb)); wo = _unit(rs, nb)
            put(name, mi, mf, wior, "bulk", n_s, n_g, wi, wo)
            # the upper hemisphere for out (where eval is non-zero)
            n_g = _unit(rs, nb); n_s = _tilt(rs, n_g, 20)
            wi = -_dir_at_cos(rs, n_g, rs.uniform(0.02, 1, nb)); wo = _dir_at_cos(rs, n_g, rs.uniform(0.02, 1, nb))
            put(name, mi, mf, wior, "bulk_upper", n_s, n_g, wi, wo)
            # cosines exactly 0, +-1e-7 .. 1e-3 (of out, then of incid), on an axis-aligned normal so that they are exact in float32
            ax = np.zeros((ne, 3)); ax[:, 1] = 1.0
            c = np.float32(rs.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-5, 1e-4, -1e-4, 1e-3, -1e-3], ne))
            wo = _dir_at_cos(rs, ax, c.astype(np.float64)); wo[:, 1] = c
            wi = -_dir_at_cos(rs, ax, rs.uniform(0.05, 1, ne))
            put(name, mi, mf, wior, "grazing_out", ax, ax, wi, wo)
            wi2 = _dir_at_cos(rs, ax, -c.astype(np.float64)); wi2[:, 1] = -c
            put(name, mi, mf, wior, "grazing_in", ax, ax, wi2, _dir_at_cos(rs, ax, rs.uniform(0.05, 1, ne)))
            # normal incidence and exit: cosines exactly +-1 (rotation_between's parallel branch, raw_of_local's sin_t <= 1e-5)
            sg = np.where(rs.uniform(size=ne) < 0.5, 1.0, -1.0)[:, None]
            n_ax = ax * sg
            put(name, mi, mf, wior, "normal_incidence", n_ax, n_ax, -n_ax, _dir_at_cos(rs, n_ax, rs.uniform(-1, 1, ne)))
            put(name, mi, mf, wior, "normal_exit", n_ax, n_ax, -_dir_at_cos(rs, n_ax, rs.uniform(0.05, 1, ne)), n_ax)
            put(name, mi, mf, wior, "normal_both", n_ax, n_ax, -n_ax, n_ax * np.where(rs.uniform(size=(ne, 1)) < 0.5, 1.0, -1.0))
            # same side: incid and out both leave (or both arrive at) the surface - eval must be 0
            n_g = _unit(rs, ne)
            wi = _dir_at_cos(rs, n_g, rs.uniform(0.02, 1, ne)); wo = _dir_at_cos(rs, n_g, rs.uniform(0.02, 1, ne))
            put(name, mi, mf, wior, "same_side", n_g, n_g, wi, wo)
            # shading normal tilted away from the geometric one by up to 60 deg
            n_g = _unit(rs, ne); n_s = _tilt(rs, n_g, 60)
            put(name, mi, mf, wior, "tilted_60", n_s, n_g, -_dir_at_cos(rs, n_g, rs.uniform(0.02, 1, ne)), _unit(rs, ne))
            # out exactly (to float32) the mirror direction of incid: the glossy peak, pow of a base near 1, the delta lobes
            # (Fresnel blend: about a shading normal 5 deg off the geometric one - along the normal its half vector's azimuth is 0 / 0)
            n_g = _unit(rs, ne); wi = -_dir_at_cos(rs, n_g, rs.uniform(0.02, 1, ne))
            refl = wi - 2 * np.sum(wi * n_g, 1, keepdims=True) * n_g
            put(name, mi, mf, wior, "mirror_peak", _tilt(rs, n_g, 5) if mi[0] == 5 and not mi[2] else n_g, n_g, wi, refl)
            # base of pow exactly 0 and tiny: out perpendicular to (modified Phong) the reflection of incid / (Blinn-Phong) the normal
            n_g = _unit(rs, ne); wi = -_dir_at_cos(rs, n_g, rs.uniform(0.3, 1, ne))
            refl = wi - 2 * np.sum(wi * n_g, 1, keepdims=True) * n_g
            a, _ = _frame(refl)
            side = a - np.sum(a * n_g, 1, keepdims=True) * n_g
            wo = _f32n(np.where(np.sum(side * n_g, 1, keepdims=True) >= 0, side, -side) + 0.3 * n_g)
            put(name, mi, mf, wior, "pow_base_zero", n_g, n_g, wi, wo)
            if bsdf:
                n = ne
                n_g = _unit(rs, n)
                for side_name, sgn in (("entering", -1.0), ("exiting", 1.0)):
                    wi = sgn * _dir_at_cos(rs, n_g, rs.uniform(0.02, 1, n))
                    wo_refl = wi - 2 * np.sum(wi * n_g, 1, keepdims=True) * n_g
                    put(name, mi, mf, wior, f"delta_reflect_{side_name}", n_g, n_g, wi, wo_refl)
                    # out = the refraction of incid (the delta transmission lobe), and the reverse pairing eval uses
                    ni, nr = (wior, float(mf[12])) if sgn < 0 else (float(mf[12]), wior)
                    dn = np.sum(wi * n_g, 1, keepdims=True)
                    cr2 = 1 - (ni / nr) ** 2 * (1 - dn * dn)
                    ok = cr2[:, 0] > 0
                    refr = (wi * (ni / nr) - n_g * (ni / nr) * dn) + n_g * np.sign(dn) * np.sqrt(np.maximum(cr2, 0))
                    refr = np.where(ok[:, None], refr, wo_refl)
                    put(name, mi, mf, wior, f"delta_refract_{side_name}", n_g, n_g, -refr, -wi)
                # within +-1e-4 rad of the critical angle (exiting the denser side only where it is denser)
                nhi, nlo = max(float(mf[12]), wior), min(float(mf[12]), wior)
                if nhi / nlo > 1.0 + 1e-6:
                    th = math.asin(nlo / nhi) + rs.uniform(-1e-4, 1e-4, n)
                    inside_mat = float(mf[12]) > wior            # the denser side: inside the material (exiting) or outside
                    c = np.cos(th)
                    wi = _dir_at_cos(rs, n_g, c if inside_mat else -c)
                    put(name, mi, mf, wior, "critical_angle", n_g, n_g, wi, wi - 2 * np.sum(wi * n_g, 1, keepdims=True) * n_g)
    out = {k: np.concatenate(v_) for k, v_ in rows_.items()}
    out["material"] = out["material"].astype(str); out["stratum"] = out["stratum"].astype(str)
    return out


def media_sweep(seed=0, n=48):
    """medium rows (med_i (n,), med_f (n,16)) and inputs in7 (n,7) = ray_in, ray_out, distance; stratum (n,) str"""
    rs = np.random.RandomState(seed)
    mi, mf, x, st = [], [], [], []

    def med(t, g=(0, 0, 0), w=(1, 0, 0), ue=(1, 1, 1), us=(0.5, 0.5, 0.5)):
        f = np.zeros(16, np.float32)
        f[0] = 1.0; f[1:4] = us; f[4:7] = np.float32(ue) - np.float32(us); f[7:10] = ue; f[10:13] = g; f[13:16] = w
        return t, f

    cases = [(f"hg_g{g:g}", med(0, (g, 0, 0))) for g in (-0.99, -0.5, 0.0, 1e-5, 0.5, 0.99)]
    cases += [("mix3", med(1, (0.7, -0.3, 0.1), (0.5, 0.3, 0.2))), ("mix2", med(1, (0.8, -0.2, 0.0), (0.7, 0.3, 0.0))),
              ("mix_w1_tiny", med(1, (0.5, 0.2, 0.9), (0.99995, 5e-5, 0.0))), ("rayleigh", med(2)), ("transparent", med(-1))]
    for name, (t, f) in cases:
        for ud in (0.0, 1e-8, 1.0, 50.0, 104.0, None):
            ri = _unit(rs, n)
            if ud is None:
                ro = _unit(rs, n); d = rs.uniform(0, 5, n)
                stn = "bulk"
            else:
                cs = rs.choice([-1.0, 1.0, 0.0, 1 - 1e-7, -1 + 1e-7, 0.5], n)
                ro = -_dir_at_cos(rs, ri, cs)
                d = np.full(n, ud)
                stn = f"ud{ud:g}"
            ff = f.copy()
            x.append(np.concatenate([_f32n(ri), _f32n(ro), d[:, None]], axis=1).astype(np.float32))
            mi.append(np.full(n, t, np.int32)); mf.append(np.repeat(ff[None], n, 0)); st.append(np.full(n, f"{name}/{stn}", object))
    return {"med_i": np.concatenate(mi), "med_f": np.concatenate(mf), "in7": np.concatenate(x), "stratum": np.concatenate(st).astype(str)}


def emitter_sweep(src_i, src_f, seed=0, n=64):
    """in11 rows (src index, hit_pos, normal, ray_d, min_depth) for every emitter of a scene: hit points near the source (the 1e-5
    clamps), across a spot's cone edge, grazing an area light and in the bulk; stratum (n,) str"""
    rs = np.random.RandomState(seed)
    X, st = [], []
    for k in range(len(src_i)):
        t = int(src_i[k][0]); pos = np.float64(src_f[k][6:9]); dr = np.float64(src_f[k][3:6]); rr = float(src_f[k][10])
        for stn in ("bulk", "near", "cone_edge", "grazing"):
            if stn == "bulk":
                hp = pos + rs.uniform(-3, 3, (n, 3))
            elif stn == "near":
                hp = pos + _unit(rs, n) * rs.choice([0.0, 1e-4, 1e-3, 3e-3, 1e-2], n)[:, None]
            elif stn == "cone_edge":
                if t != 2:
                    continue
                c = rr + rs.uniform(-1e-4, 1e-4, n)
                hp = pos + _dir_at_cos(rs, np.repeat(dr[None], n, 0), c) * rs.uniform(0.5, 3, n)[:, None]
            else:
                hp = pos + _unit(rs, n) * rs.uniform(0.5, 3, n)[:, None]
            nrm = _unit(rs, n)
            if stn == "grazing":
                rd = _dir_at_cos(rs, nrm, rs.choice([0.0, 1e-6, -1e-6, 1e-3, -1e-3], n))
            else:
                rd = _unit(rs, n)
            md = rs.uniform(0.05, 6, n) if stn != "near" else rs.choice([1e-6, 1e-3, 0.1, 1.0], n)
            X.append(np.concatenate([np.full((n, 1), k), hp, _f32n(nrm), _f32n(rd), md[:, None]], axis=1).astype(np.float32))
            st.append(np.full(n, f"src{k}_t{t}/{stn}", object))
    return np.concatenate(X), np.concatenate(st).astype(str)


def emitter_sample_sweep(scene, seed=0, n=64):
    """hit points for emitter_sample_hit, aimed at every emitter's own edges -> rows (m,4) float32 = (src index, hit_pos), stratum (m,)
    str = "src<k>_<kind>/<stratum>", on_edge (m,) bool.  `scene`: prims, normals, obj_info, src_i, src_f as adapt_amd.scene_pack packs
    them.  Offsets at an area light are relative to its extent (a mesh's largest box side, a sphere's radius).  The rows flagged on_edge
    sit ON a float32 decision (height 0 over a mesh light, its vertices, a sphere's centre, a beam's axis, a cone's cosine): float32
    decides them either way, and they are held to the two-branch rule (tests/emitter_cases.py), never left out."""
    rs = np.random.RandomState(seed)
    X, st, edge = [], [], []

    def put(k, kind, name, hp, on_edge=False):
        hp = np.asarray(hp, np.float64).reshape(-1, 3)
        X.append(np.concatenate([np.full((len(hp), 1), k), hp], axis=1).astype(np.float32))
        st.append(np.full(len(hp), f"src{k}_{kind}/{name}", object)); edge.append(np.full(len(hp), on_edge))

    pick = lambda vals: rs.choice(vals, n)[:, None]
    for k in range(len(scene.src_i)):
        t = int(scene.src_i[k][0])
        sf = np.float64(scene.src_f[k])
        pos, dr, rr = sf[6:9], sf[3:6], float(sf[10])
        geom = emitter_geom(scene, k)
        kind = emitter_kind(t, geom)
        if kind == "mesh":
            dv1, dv2, v0, nrm = (np.float64(a) for a in geom[1:])
            verts = np.concatenate([v0, v0 + dv1, v0 + dv2])
            cen, ext = 0.5 * (verts.min(0) + verts.max(0)), float((verts.max(0) - verts.min(0)).max())
            nn = np.repeat(nrm[:1], n, 0)
            ta, tb = _frame(nn)
            over = lambda w: cen + ext * (rs.uniform(-w, w, (n, 1)) * ta + rs.uniform(-w, w, (n, 1)) * tb)
            put(k, kind, "bulk", cen + ext * _unit(rs, n) * rs.uniform(0.3, 6, (n, 1)))
            put(k, kind, "plane", over(0.75) + nn * ext * pick([1e-5, -1e-5, 1e-4, -1e-4, 1e-2, -1e-2]))
            put(k, kind, "behind", over(0.75) - nn * ext * rs.uniform(0.1, 3, (n, 1)))
            put(k, kind, "front_close", over(0.4) + nn * ext * 10.0 ** rs.uniform(-3, -1, (n, 1)))
            put(k, kind, "far", cen + 1e3 * ext * _dir_at_cos(rs, nn, rs.uniform(0.05, 1, n)))
            put(k, kind, "edge_height0", over(0.3), True)
            put(k, kind, "edge_vertex", verts[rs.randint(0, len(verts), n)], True)
        elif kind == "sphere":
            cen, rad = np.float64(geom[1]), abs(geom[2])
            put(k, kind, "bulk", cen + rad * _unit(rs, n) * rs.uniform(1.2, 6, (n, 1)))
            put(k, kind, "skin", cen + rad * _unit(rs, n) * (1.0 + pick([1e-4, 1e-2])))
            put(k, kind, "inside", cen + rad * _unit(rs, n) * rs.uniform(0.01, 0.99, (n, 1)))
            ang = rs.choice([2e-3, 4e-3, 5e-3, 1e-2, 0.1], n)
            ax = np.zeros((n, 3)); ax[:, 1] = rs.choice([-1.0, 1.0], n)
            put(k, kind, "pole", cen + rad * _dir_at_cos(rs, ax, np.cos(ang)) * rs.uniform(1.5, 4, (n, 1)))
            put(k, kind, "edge_centre", np.repeat(cen[None], 8, 0), True)
        elif kind in ("point", "spot"):
            put(k, kind, "bulk", pos + rs.uniform(-3, 3, (n, 3)))
            put(k, kind, "near", pos + _unit(rs, n) * pick([0.0, 1e-4, 1e-3, 1e-2, 0.9, 1.1]))
            if kind == "spot":
                axis = np.repeat(dr[None], n, 0)
                put(k, kind, "cone_edge", pos + _dir_at_cos(rs, axis, rr + rs.choice([-1.0, 1.0], n) * rs.uniform(2e-5, 1e-4, n)) * rs.uniform(0.5, 3, (n, 1)))
                put(k, kind, "edge_cone", pos + _dir_at_cos(rs, axis, np.full(n, rr)) * rs.uniform(0.5, 3, (n, 1)), True)
        else:
            axis = np.repeat(dr[None], n, 0)
            ta, tb = _frame(axis)
            phi = rs.uniform(0, 2 * np.pi, (n, 1))
            radial = np.cos(phi) * ta + np.sin(phi) * tb
            put(k, kind, "bulk", pos + rs.uniform(-3, 3, (n, 3)))
            # (along the beam by no more than two radii: the float32 error of dist grows with |to_hit|^2 / dist, and 1e-5 must stay decidable)
            put(k, kind, "rim", pos + axis * (rr if rr > 0 else 0.25) * rs.uniform(0.2, 2, (n, 1)) + radial * np.abs(rr + pick([1e-5, -1e-5, 1e-4, -1e-4])))
            put(k, kind, "base", pos + axis * pick([1e-5, -1e-5, 1e-3, -1e-3]) + radial * rr * rs.uniform(0, 0.9, (n, 1)))
            put(k, kind, "edge_axis", pos + axis * rs.uniform(0.5, 2, (n, 1)) + radial * pick([0.0, 1e-7, 1e-5]), True)
    return np.concatenate(X), np.concatenate(st).astype(str), np.concatenate(edge)
