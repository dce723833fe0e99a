// occ_beam.hpp -- complete candidate lists of the any-hit occluder table's keys (DESIGN.md section 2
// and 5, "complete keys").  A key of the table is (origin cell of the root box, direction bin of a
// cube-map face).  Its beam is the cell's box and one interval per direction component; the functions
// here list every triangle that a ray of the beam could be accepted on by the any-hit traversal, with
// the interval machinery of primary_beam.hpp (each fp32 operation of the slab test, the cull and the
// determinant is monotone in its operands).  A key whose list fits the table entry is complete: a ray
// that lies in the beam (occ_member, the same intervals), has a finite inverse direction and a
// positive culling scale is occluded iff one of the listed triangles passes occ_test.
// Whether a ray's key, as occ_index computes it, is the key whose beam contains the ray is not
// assumed anywhere: k_material tests the membership per ray, so the bin intervals below only decide
// how many rays can be resolved, never a result.
// __host__ __device__: tests/native/occ_beam.cpp runs the builder on the CPU.
#pragma once
#include "primary_beam.hpp"

namespace mcpt {

// Entry words of a complete key: bit 31 with a triangle record index below 2^24, or the marked empty
// word.  A plain store of a record index (k_trace's occluder records) clears bit 31, so an entry some
// ray has written to is no longer complete; kOccEmpty (all ones) is not a complete word either.
constexpr uint32_t kOccDoneBit = 0x80000000u;
constexpr uint32_t kOccDoneNone = 0x81000000u;  // index field 2^24: beyond every record
constexpr uint32_t kOccDoneIndex = 0x01ffffffu;
MCPT_HD bool occ_word_done(uint32_t w) { return (w >> 25) == 0x40u; }

// The origin grid and the direction-bin table of a scene's occluder table: cell c of axis k spans
// [mn[k] + c cell[k], mn[k] + (c + 1) cell[k]]; dir holds, per (face * b + ub) * b + vb, the
// intervals of occ_dir_bin as two float4: {d.x lo, hi, d.y lo, hi} {d.z lo, hi, 0, 0}.
struct OccGrid {
    float mn[3], cell[3];
    int g, b;
    const float4* dir;
};
constexpr int kOccDirF4 = 2;

// Direction-component intervals of bin (ub, vb) of a face (0 / 1: +x / -x major with (u, v) = (d.y,
// d.z); 2 / 3: y major, (d.x, d.z); 4 / 5: z major, (d.x, d.y)), for directions of length 1 +- 1e-4
// whose cube-map coordinates u / |major|, v / |major| fall in the bin (widened by 1e-5: the bin
// index's rcp and rounding; not across zero: a bin edge at zero stays there, so the component's sign
// is known and the axis constrains the slab test, occ_inv_axis).  Evaluated in double and rounded to
// float; nothing depends on the rounding (see the header).
MCPT_HD void occ_dir_bin(int B, uint32_t face, uint32_t ub, uint32_t vb, float* out) {
    const double hb = 0.5 * (double)B, s = 1e-5;
    auto edge = [&](double e, double w) { return e == 0.0 ? 0.0 : e + w; };
    const double a0 = edge(((double)ub - hb) / hb, -s), a1 = edge(((double)ub + 1.0 - hb) / hb, s);
    const double b0 = edge(((double)vb - hb) / hb, -s), b1 = edge(((double)vb + 1.0 - hb) / hb, s);
    const double a2lo = (a0 <= 0.0 && a1 >= 0.0) ? 0.0 : (a0 * a0 < a1 * a1 ? a0 * a0 : a1 * a1);
    const double a2hi = a0 * a0 > a1 * a1 ? a0 * a0 : a1 * a1;
    const double b2lo = (b0 <= 0.0 && b1 >= 0.0) ? 0.0 : (b0 * b0 < b1 * b1 ? b0 * b0 : b1 * b1);
    const double b2hi = b0 * b0 > b1 * b1 ? b0 * b0 : b1 * b1;
    const double mlo = (1.0 - 1e-4) / __builtin_sqrt(1.0 + a2hi + b2hi), mhi = (1.0 + 1e-4) / __builtin_sqrt(1.0 + a2lo + b2lo);
    auto hull = [&](double r0, double r1, double& lo, double& hi) {
        const double p[4] = {r0 * mlo, r0 * mhi, r1 * mlo, r1 * mhi};
        lo = hi = p[0];
        for (int k = 1; k < 4; k++) { lo = p[k] < lo ? p[k] : lo; hi = p[k] > hi ? p[k] : hi; }
    };
    double ulo, uhi, vlo, vhi;
    hull(a0, a1, ulo, uhi);
    hull(b0, b1, vlo, vhi);
    const double jlo = (face & 1u) ? -mhi : mlo, jhi = (face & 1u) ? -mlo : mhi;
    double lo[3], hi[3];
    const int major = (int)(face >> 1), ua = major == 0 ? 1 : 0, va = major == 2 ? 1 : 2;
    lo[major] = jlo; hi[major] = jhi;
    lo[ua] = ulo; hi[ua] = uhi;
    lo[va] = vlo; hi[va] = vhi;
    for (int k = 0; k < 3; k++) { out[2 * k] = (float)lo[k]; out[2 * k + 1] = (float)hi[k]; }
}
inline void occ_dir_table(int B, float4* out) {  // 6 B B bins, kOccDirF4 float4 each
    for (uint32_t f = 0; f < 6u; f++)
        for (uint32_t u = 0; u < (uint32_t)B; u++)
            for (uint32_t v = 0; v < (uint32_t)B; v++) {
                float t[6];
                occ_dir_bin(B, f, u, v, t);
                float4* o = out + kOccDirF4 * ((f * B + u) * (size_t)B + v);
                o[0] = float4{t[0], t[1], t[2], t[3]};
                o[1] = float4{t[4], t[5], 0.f, 0.f};
            }
}

MCPT_HD Iv occ_cell_iv(float mn, float cell, uint32_t c) { return iv_fix(mn + (float)c * cell, mn + (float)(c + 1u) * cell); }
// The beam of key (cell cx cy cz, direction bin dirbin = (face * b + ub) * b + vb)
MCPT_HD Beam occ_key_beam(const OccGrid& g, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t dirbin) {
    const float4* t = g.dir + kOccDirF4 * (size_t)dirbin;
    const float4 t0 = t[0], t1 = t[1];
    Beam b;
    b.o = Iv3{occ_cell_iv(g.mn[0], g.cell[0], cx), occ_cell_iv(g.mn[1], g.cell[1], cy), occ_cell_iv(g.mn[2], g.cell[2], cz)};
    b.d = Iv3{iv_fix(t0.x, t0.y), iv_fix(t0.z, t0.w), iv_fix(t1.x, t1.y)};
    b.ok = true;
    return b;
}
MCPT_HD bool iv_in(Iv a, float v) { return a.lo <= v && v <= a.hi; }  // false for a NaN v
MCPT_HD bool beam_contains(const Beam& b, V3 o, V3 d) {
    return iv_in(b.o.x, o.x) && iv_in(b.o.y, o.y) && iv_in(b.o.z, o.z) && iv_in(b.d.x, d.x) && iv_in(b.d.y, d.y) &&
           iv_in(b.d.z, d.z);
}
// true: ray (o, d) is a ray of the key's beam (k_material's run-time membership test)
MCPT_HD bool occ_member(const OccGrid& g, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t dirbin, V3 o, V3 d) {
    return beam_contains(occ_key_beam(g, cx, cy, cz, dirbin), o, d);
}

// 1 / d of one axis for the beam's rays with a finite inverse direction.  Where beam_inv_axis gives up on
// an interval that touches zero, an interval with zero at one end still constrains those rays: their
// component is not zero and |1 / d| <= FLT_MAX, so 1 / d lies between the other end's reciprocal and
// +-FLT_MAX (a reciprocal that overflows is clamped the same way: the division is monotone).
MCPT_HD void occ_inv_axis(Iv d, Iv& inv, bool& con) {
    const float big = 3.4028235e38f;
    inv = iv_all();
    con = false;
    if (d.lo >= 0.f && d.hi > 0.f) {
        inv = iv_fix(__builtin_fminf(1.f / d.hi, big), d.lo > 0.f ? __builtin_fminf(1.f / d.lo, big) : big);
        con = true;
    } else if (d.hi <= 0.f && d.lo < 0.f) {
        inv = iv_fix(d.hi < 0.f ? __builtin_fmaxf(1.f / d.hi, -big) : -big, __builtin_fmaxf(1.f / d.lo, -big));
        con = true;
    }
}
MCPT_HD BeamInv occ_beam_inv(const Beam& b) {
    BeamInv r;
    occ_inv_axis(b.d.x, r.x, r.cx);
    occ_inv_axis(b.d.y, r.y, r.cy);
    occ_inv_axis(b.d.z, r.z, r.cz);
    return r;
}

// Bounds of the slab test's entry and exit over the beam (beam_misses_box's t0 / t1): every ray of
// the beam with a finite inverse direction has t0 >= t0lo and t1 <= t1hi for this box (an axis the
// beam does not constrain is left out, which only loosens both).
MCPT_HD void beam_box_range(const Beam& b, const BeamInv& iv, float mnx, float mny, float mnz, float mxx, float mxy,
                            float mxz, float& t0lo, float& t1hi) {
    float t0 = -__builtin_huge_valf(), t1 = __builtin_huge_valf(), e, x;
    if (iv.cx) { beam_slab_axis(mnx, mxx, b.o.x, iv.x, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    if (iv.cy) { beam_slab_axis(mny, mxy, b.o.y, iv.y, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    if (iv.cz) { beam_slab_axis(mnz, mxz, b.o.z, iv.z, e, x); t0 = __builtin_fmaxf(t0, e); t1 = __builtin_fminf(t1, x); }
    t0lo = t0;
    t1hi = t1;
}
// Upper bound of the positive culling scales of the beam's rays (kernels.hip cull_iota: iota = max_a
// |1 / d_a| (1 + 2^-18), returned positive only when iota P <= 1).  |1 / d_a| <= 1 / min |d_a| for a
// component interval without zero (the division is monotone), and RN(iota P) <= 1 gives iota <=
// (1 + 2^-24) / P < RN(1 / P) 1.000001.  +inf when neither bounds it.
MCPT_HD float beam_iota_hi(const BeamInv& iv, float cull_p) {
    float m = __builtin_huge_valf();
    if (iv.cx && iv.cy && iv.cz) {
        const float ax = __builtin_fmaxf(__builtin_fabsf(iv.x.lo), __builtin_fabsf(iv.x.hi));
        const float ay = __builtin_fmaxf(__builtin_fabsf(iv.y.lo), __builtin_fabsf(iv.y.hi));
        const float az = __builtin_fmaxf(__builtin_fabsf(iv.z.lo), __builtin_fabsf(iv.z.hi));
        m = __builtin_fmaxf(__builtin_fmaxf(ax, ay), az) * kCullSlackF;
    }
    if (cull_p > 0.f) m = __builtin_fminf(m, (1.f / cull_p) * 1.000001f);
    return m;
}
// The interval form of keep_box's behind cut (kernels.hip; any-hit rays: cut = +inf).  true: every
// ray of the beam with a positive culling scale io <= io_hi culls the box of margin w whose exit is
// at most t1hi: its m = w io lies in [0, w io_hi] and its t1 <= t1hi, and fma is monotone, so
// fma(t1, 1 - 2^-18, m) <= fma(t1hi, 1 - 2^-18, w io_hi) < 0.  A NaN or negative margin keeps the box.
MCPT_HD bool beam_behind_box(float t1hi, float w, float io_hi) {
    const float m = w * io_hi;
    return m >= 0.f && __builtin_fmaf(t1hi, kCullBehindF, m) < 0.f;
}

// The child-pair tree the builder walks (kernels.hpp DevScene: pair nodes of 4 float4 -- per axis
// (mn0, mn1, mx0, mx1), then (ref0, ref1, margin0, margin1); a ref >= 0 is a pair node, < 0 a leaf
// 0x80000000 | (count - 1) << 24 | offset, -1 no child) and the triangle records (tri_f4 float4
// each: (v0.xyz, e1.x) (e1.yz, e2.xy) (e2.z, ..)).
struct OccTree {
    const float4* nodes;
    const float4* tri;
    int tri_f4;
    uint32_t ntri;
    int root_ref;
    float root_mn[3], root_mx[3];
    float root_w, cull_p;
};
constexpr int kOccListStack = 64;    // the traversal's own bound on the tree's depth
constexpr int kOccListBudget = 768;  // boxes tested per key before the key is given up (left dynamic)

// The candidate list of a beam: every triangle record that a ray of the beam with a finite inverse
// direction and a positive culling scale can be accepted on.  A subtree is dropped when every such
// ray fails its box's slab test or culls the box as behind the origin (a leaf's box and margin are
// its parent's entries for it; every ancestor's box contains the leaf's and its margin is no
// smaller, so a ray that drops an ancestor drops the leaf's box too); a triangle when every ray
// rejects it as back-facing.  Returns the number of candidates written to out (<= ways), or -1 when
// there are more, the box budget ran out or the stack would overflow.
MCPT_HD int occ_key_list(const OccTree& t, const Beam& b, int ways, uint32_t* out) {
    const BeamInv iv = occ_beam_inv(b);
    const float io_hi = beam_iota_hi(iv, t.cull_p);
    int stack[kOccListStack];
    int sp = 0, n = 0, budget = kOccListBudget;
    // one box: 1 push its node, 0 dropped or a leaf taken, -1 give up
    auto visit = [&](int ref, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float w) -> int {
        if (ref == -1) return 0;
        if (--budget < 0) return -1;
        float t0lo, t1hi;
        beam_box_range(b, iv, mnx, mny, mnz, mxx, mxy, mxz, t0lo, t1hi);
        if (t0lo > t1hi || beam_behind_box(t1hi, w, io_hi)) return 0;
        if (ref >= 0) {
            if (sp >= kOccListStack) return -1;
            stack[sp++] = ref;
            return 1;
        }
        const uint32_t off = (uint32_t)ref & 0xffffffu, cnt = (((uint32_t)ref >> 24) & 7u) + 1u;
        for (uint32_t k = off; k < off + cnt && k < t.ntri; k++) {
            const float4* r = t.tri + (size_t)t.tri_f4 * k;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            if (beam_backfacing(b, v3(r0.w, r1.x, r1.y), v3(r1.z, r1.w, r2.x))) continue;
            if (n >= ways) return -1;
            out[n++] = k;
        }
        return 0;
    };
    if (visit(t.root_ref, t.root_mn[0], t.root_mn[1], t.root_mn[2], t.root_mx[0], t.root_mx[1], t.root_mx[2], t.root_w) < 0)
        return -1;
    while (sp > 0) {
        const float4* nd = t.nodes + 4 * (size_t)stack[--sp];
        const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        if (visit(__builtin_bit_cast(int, q3.x), q0.x, q1.x, q2.x, q0.z, q1.z, q2.z, q3.z) < 0) return -1;
        if (visit(__builtin_bit_cast(int, q3.y), q0.y, q1.y, q2.y, q0.w, q1.w, q2.w, q3.w) < 0) return -1;
    }
    return n;
}

}  // namespace mcpt
