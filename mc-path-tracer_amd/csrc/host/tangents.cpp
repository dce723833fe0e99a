// tangents.cpp -- vertex tangents from texture coordinates for normal maps (DESIGN.md section 21;
// mcpt_tangents_from_uv, include/mcpt.h states the arithmetic).  Host only: no device call.  All double on
// the float inputs, one operation per statement's node in the stated order; the build compiles host code
// with -ffp-contract=off, so tests/texture_nrm_ref.py's numpy float64 restatement matches bit for bit
// after the rounding to float.
#include <cmath>

#include "mcpt.h"

namespace {

struct D3 {
    double x, y, z;
};
inline D3 ld(const float* p, int32_t t) { return D3{(double)p[3 * (size_t)t], (double)p[3 * (size_t)t + 1], (double)p[3 * (size_t)t + 2]}; }
inline D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 mul(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
inline double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// normalize(cross(N, axis of N's smallest component in magnitude, the first on a tie)); (1, 0, 0) where that
// cross has no finite non-zero length
D3 fallback(D3 N) {
    const double a[3] = {std::fabs(N.x), std::fabs(N.y), std::fabs(N.z)};
    int k = a[1] < a[0] ? 1 : 0;
    if (a[2] < a[k]) k = 2;
    const D3 ax{k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    const D3 q = cross(N, ax);
    const double l = std::sqrt(dot(q, q));
    if (!(std::isfinite(l) && l > 0.0)) return D3{1.0, 0.0, 0.0};
    return D3{q.x / l, q.y / l, q.z / l};
}

}  // namespace

extern "C" int mcpt_tangents_from_uv(int32_t ntri, const float* v0, const float* v1, const float* v2, const float* n0,
                                     const float* n1, const float* n2, const float* uv0, const float* uv1, const float* uv2,
                                     float* tan0, float* tan1, float* tan2) {
    if (ntri < 0) return MCPT_E_INVALID;
    if (ntri > 0 && (!v0 || !v1 || !v2 || !n0 || !n1 || !n2 || !uv0 || !uv1 || !uv2 || !tan0 || !tan1 || !tan2)) return MCPT_E_INVALID;
    const float* nn[3] = {n0, n1, n2};
    float* out[3] = {tan0, tan1, tan2};
    for (int32_t t = 0; t < ntri; t++) {
        const D3 p0 = ld(v0, t);
        const D3 e1 = sub(ld(v1, t), p0), e2 = sub(ld(v2, t), p0);
        const double u0 = uv0[2 * (size_t)t], w0 = uv0[2 * (size_t)t + 1];
        const double du1 = (double)uv1[2 * (size_t)t] - u0, dv1 = (double)uv1[2 * (size_t)t + 1] - w0;
        const double du2 = (double)uv2[2 * (size_t)t] - u0, dv2 = (double)uv2[2 * (size_t)t + 1] - w0;
        const double det = du1 * dv2 - du2 * dv1;
        const double r = 1.0 / det;
        const D3 Tt = mul(sub(mul(e1, dv2), mul(e2, dv1)), r);
        const D3 Bt = mul(sub(mul(e2, du1), mul(e1, du2)), r);
        const bool det_ok = std::isfinite(det) && det != 0.0;
        for (int i = 0; i < 3; i++) {
            const D3 N = ld(nn[i], t);
            const D3 q = sub(Tt, mul(N, dot(N, Tt)));
            const double l = std::sqrt(dot(q, q));
            D3 T;
            double s = 1.0;
            if (det_ok && std::isfinite(l) && l > 0.0) {
                T = D3{q.x / l, q.y / l, q.z / l};
                if (dot(cross(N, T), Bt) < 0.0) s = -1.0;
            } else {
                T = fallback(N);
            }
            float* o = out[i] + 4 * (size_t)t;
            o[0] = (float)T.x, o[1] = (float)T.y, o[2] = (float)T.z, o[3] = (float)s;
        }
    }
    return MCPT_OK;
}
