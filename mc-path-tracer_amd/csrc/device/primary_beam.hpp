// primary_beam.hpp -- interval bounds of a pixel's primary rays ("the primary
// beam").  Every sample of a pixel runs gen_ray_lens (mcpt_core.hpp) with the same focal point and
// two lens draws |lx|, |ly| <= lens_radius.  The functions here push those two intervals through
// the very fp32 expressions gen_ray_lens and the slab test evaluate.  Each operation involved (add,
// sub, mul, div, sqrt) is correctly rounded, hence monotone in each operand: the value computed
// from operands inside their intervals lies between the values computed at the interval end
// points.  No geometric epsilon is involved; the bound holds for the computed floats themselves.
// __host__ __device__: tests/native/primary_beam.cpp checks the containment on the CPU.
#pragma once
#include "mcpt_core.hpp"

namespace mcpt {

struct Iv { float lo, hi; };  // lo <= hi, never NaN (an undefined bound is widened to +-inf)
struct Iv3 { Iv x, y, z; };

MCPT_HD Iv iv_all() { return Iv{-__builtin_huge_valf(), __builtin_huge_valf()}; }
MCPT_HD Iv iv_pt(float v) { return v == v ? Iv{v, v} : iv_all(); }
MCPT_HD Iv iv_fix(float lo, float hi) { return (lo <= hi) ? Iv{lo, hi} : iv_all(); }  // NaN end point: everything
MCPT_HD Iv iv_add(Iv a, Iv b) { return iv_fix(a.lo + b.lo, a.hi + b.hi); }
MCPT_HD Iv iv_sub(Iv a, Iv b) { return iv_fix(a.lo - b.hi, a.hi - b.lo); }
MCPT_HD Iv iv_hull4(float p0, float p1, float p2, float p3) {
    if (!(p0 == p0 && p1 == p1 && p2 == p2 && p3 == p3)) return iv_all();
    const float lo = __builtin_fminf(__builtin_fminf(p0, p1), __builtin_fminf(p2, p3));
    const float hi = __builtin_fmaxf(__builtin_fmaxf(p0, p1), __builtin_fmaxf(p2, p3));
    return Iv{lo, hi};
}
MCPT_HD Iv iv_mul(Iv a, Iv b) { return iv_hull4(a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi); }
MCPT_HD Iv iv_scale(float c, Iv a) { return iv_hull4(c * a.lo, c * a.hi, c * a.lo, c * a.hi); }
MCPT_HD bool iv_has0(Iv a) { return !(a.lo > 0.f || a.hi < 0.f); }
// a / b for b without zero (the caller checks)
MCPT_HD Iv iv_div(Iv a, Iv b) { return iv_hull4(a.lo / b.lo, a.lo / b.hi, a.hi / b.lo, a.hi / b.hi); }
MCPT_HD Iv iv_sqr(Iv a) {  // x * x: monotone in |x|
    if (a.lo >= 0.f) return iv_fix(a.lo * a.lo, a.hi * a.hi);
    if (a.hi <= 0.f) return iv_fix(a.hi * a.hi, a.lo * a.lo);
    return iv_fix(0.f, __builtin_fmaxf(a.lo * a.lo, a.hi * a.hi));
}
MCPT_HD Iv iv_sqrt(Iv a) { return iv_fix(__builtin_sqrtf(a.lo), __builtin_sqrtf(a.hi)); }  // a.lo >= 0

// The rays of one pixel: origin and direction intervals; ok = false when no bound could be given
// (a projective divide or a normalisation whose denominator interval touches zero).
struct Beam { Iv3 o, d; bool ok; };

// concentric_disk returns rr * (cos, sin) with |rr| <= 1 and cephes polynomials within an ulp of
// [-1, 1]: |lx| = |RN(dx * R)| <= R (1 + 1e-5) with room to spare for a normal R.  Near the bottom of
// the float range the product R * 1.00001f rounds back to R, so the bound is also at least the fourth
// float above R (a subnormal R: |RN(dx R)| <= R + 1 ulp).
constexpr float kBeamLensSlack = 1.00001f;
MCPT_HD float beam_lens_bound(float R) {  // R > 0
    const float up = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, R) + 4u);  // R finite: 4 floats up (or inf)
    return __builtin_fmaxf(R * kBeamLensSlack, up);
}

// gen_ray_lens(c, pFocal, .) for every lens draw
MCPT_HD Beam beam_lens(const CamView& c, V3 pFocal) {
    Beam b;
    b.ok = false;
    const float R = beam_lens_bound(c.lens_radius);
    const Iv L = iv_fix(-R, R);
    Iv al[4];
    for (int r = 0; r < 4; r++) {  // mat_vec4(c.iv, lx, ly, 0, 1): ((m0 lx + m1 ly) + m2 0) + m3 1
        Iv s = iv_add(iv_scale(c.iv[0 * 4 + r], L), iv_scale(c.iv[1 * 4 + r], L));
        s = iv_add(s, iv_pt(c.iv[2 * 4 + r] * 0.f));
        al[r] = iv_add(s, iv_pt(c.iv[3 * 4 + r] * 1.f));
    }
    if (iv_has0(al[3])) return b;
    b.o.x = iv_div(al[0], al[3]);  // quot3: RN32(a / b)
    b.o.y = iv_div(al[1], al[3]);
    b.o.z = iv_div(al[2], al[3]);
    const Iv vx = iv_sub(iv_pt(pFocal.x), b.o.x), vy = iv_sub(iv_pt(pFocal.y), b.o.y), vz = iv_sub(iv_pt(pFocal.z), b.o.z);
    const Iv n2 = iv_add(iv_add(iv_sqr(vx), iv_sqr(vy)), iv_sqr(vz));  // dot(v, v)
    if (!(n2.lo > 0.f)) return b;
    const Iv l = iv_sqrt(n2);
    if (!(l.lo > 0.f)) return b;  // normalize() leaves a zero-length v as it is
    b.d.x = iv_div(vx, l);
    b.d.y = iv_div(vy, l);
    b.d.z = iv_div(vz, l);
    b.ok = true;
    return b;
}
// the pinhole ray of a pixel: a beam of one ray
MCPT_HD Beam beam_point(V3 o, V3 d) {
    Beam b;
    b.o = Iv3{iv_pt(o.x), iv_pt(o.y), iv_pt(o.z)};
    b.d = Iv3{iv_pt(d.x), iv_pt(d.y), iv_pt(d.z)};
    b.ok = true;
    return b;
}

// 1 / d per axis.  con: the axis constrains the slab test -- its direction interval excludes zero
// and both reciprocals are finite.  An axis that is not constrained is dropped from the test, which
// can only make it pass more.
struct BeamInv { Iv x, y, z; bool cx, cy, cz; };
MCPT_HD void beam_inv_axis(Iv d, Iv& inv, bool& con) {
    inv = iv_all();
    con = false;
    if (iv_has0(d)) return;
    const float a = 1.f / d.hi, b = 1.f / d.lo;  // 1 / x decreases on either side of zero
    if (!(__builtin_fabsf(a) < __builtin_huge_valf() && __builtin_fabsf(b) < __builtin_huge_valf())) return;
    inv = iv_fix(a, b);
    con = true;
}
MCPT_HD BeamInv beam_inv(const Beam& b) {
    BeamInv r;
    beam_inv_axis(b.d.x, r.x, r.cx);
    beam_inv_axis(b.d.y, r.y, r.cy);
    beam_inv_axis(b.d.z, r.z, r.cz);
    return r;
}

// One axis of the slab test for the whole beam: the products (mn - o) inv and (mx - o) inv as
// intervals; the ray's entry is the smaller product and its exit the larger, so entry >= lo of both
// minima and exit <= hi of both maxima.
MCPT_HD void beam_slab_axis(float mn, float mx, Iv o, Iv inv, float& entry_lo, float& exit_hi) {
    const Iv a = iv_mul(iv_sub(iv_pt(mn), o), inv), b = iv_mul(iv_sub(iv_pt(mx), o), inv);
    entry_lo = __builtin_fminf(a.lo, b.lo);
    exit_hi = __builtin_fmaxf(a.hi, b.hi);
}
// true: every ray of the beam with a finite inverse direction fails the slab test t0 <= t1 of this
// box (pair_slab's arithmetic: t0 = max of the per-axis entries, t1 = min of the exits).  A NaN box
// coordinate widens its products to everything and the box is kept.
MCPT_HD bool beam_misses_box(const Beam& b, const BeamInv& iv, float mnx, float mny, float mnz, float mxx, float mxy,
                             float mxz) {
    float t0 = -__builtin_huge_valf(), t1 = __builtin_huge_valf(), e, x;
    if (iv.cx) { beam_slab_axis(mnx, mxx, b.o.x, iv.x, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    if (iv.cy) { beam_slab_axis(mny, mxy, b.o.y, iv.y, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    if (iv.cz) { beam_slab_axis(mnz, mxz, b.o.z, iv.z, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    return t0 > t1;
}
// true: tri_test's determinant dot(e1, cross(d, e2)) is below K_EPSILON for every ray of the beam
// (the triangle is rejected as back-facing or edge-on by all of them)
MCPT_HD bool beam_backfacing(const Beam& b, V3 e1, V3 e2) {
    const Iv px = iv_sub(iv_scale(e2.z, b.d.y), iv_scale(e2.y, b.d.z));  // d.y e2.z - d.z e2.y
    const Iv py = iv_sub(iv_scale(e2.x, b.d.z), iv_scale(e2.z, b.d.x));
    const Iv pz = iv_sub(iv_scale(e2.y, b.d.x), iv_scale(e2.x, b.d.y));
    const Iv det = iv_add(iv_add(iv_scale(e1.x, px), iv_scale(e1.y, py)), iv_scale(e1.z, pz));
    return det.hi < K_EPSILON;
}

}  // namespace mcpt
