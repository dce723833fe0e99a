// Host check of the primary beam's interval bounds (device/primary_beam.hpp): for random cameras,
// pixels and lens draws, the ray gen_ray_lens computes -- origin, direction and inverse direction --
// lies inside the pixel's intervals, a box the beam "provably misses" fails the slab test for that
// ray, and a triangle the beam sees back-facing has det < K_EPSILON for it.  Prints "bad=N".
#include <cmath>
#include <cstdio>
#include <cstring>

#include "device/primary_beam.hpp"

using namespace mcpt;

static uint64_t g_s = 0x1234567ull;
static double urand() {
    g_s = splitmix64(g_s);
    return (double)(g_s >> 11) * (1.0 / 9007199254740992.0);
}
static double srand1() { return 2.0 * urand() - 1.0; }

// column-major m[c * 4 + r]
static void mul4(const double* a, const double* b, double* o) {
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += a[k * 4 + r] * b[c * 4 + k];
            o[c * 4 + r] = s;
        }
}
static bool inv4(const double* m, double* o) {
    double a[4][8];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) { a[r][c] = m[c * 4 + r]; a[r][4 + c] = r == c; }
    for (int i = 0; i < 4; i++) {
        int p = i;
        for (int r = i + 1; r < 4; r++) if (std::fabs(a[r][i]) > std::fabs(a[p][i])) p = r;
        if (std::fabs(a[p][i]) < 1e-12) return false;
        for (int c = 0; c < 8; c++) { double t = a[i][c]; a[i][c] = a[p][c]; a[p][c] = t; }
        const double d = a[i][i];
        for (int c = 0; c < 8; c++) a[i][c] /= d;
        for (int r = 0; r < 4; r++)
            if (r != i) { const double f = a[r][i]; for (int c = 0; c < 8; c++) a[r][c] -= f * a[i][c]; }
    }
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) o[c * 4 + r] = a[r][4 + c];
    return true;
}
// a look-at camera: eye, yaw / pitch in radians; axis = true: looking exactly down -z
static bool make_cam(CamView& cv, const double eye[3], double yaw, double pitch, bool axis, float lens, float focal) {
    double f[3] = {std::cos(yaw) * std::cos(pitch), std::sin(pitch), std::sin(yaw) * std::cos(pitch)};
    if (axis) { f[0] = 0; f[1] = 0; f[2] = -1; }
    double up[3] = {0, 1, 0}, s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (double& v : s) v /= sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    double view[16] = {s[0], u[0], -f[0], 0, s[1], u[1], -f[1], 0, s[2], u[2], -f[2], 0,
                       -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]), -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]),
                       f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2], 1};
    const double t = std::tan(0.5 * 0.785398), asp = 16.0 / 9.0, zn = 0.01, zf = 1e4;
    double proj[16] = {0};
    proj[0] = 1 / (asp * t);
    proj[5] = 1 / t;
    proj[10] = -(zf + zn) / (zf - zn);
    proj[11] = -1;
    proj[14] = -2 * zf * zn / (zf - zn);
    double pv[16], ipv[16], iv[16];
    mul4(proj, view, pv);
    if (!inv4(pv, ipv) || !inv4(view, iv)) return false;
    for (int i = 0; i < 16; i++) { cv.ivp[i] = (float)ipv[i]; cv.iv[i] = (float)iv[i]; }
    cv.lens_radius = lens;
    cv.focal = focal;
    return true;
}
static bool in(Iv a, float v) { return a.lo <= v && v <= a.hi; }

int main() {
    long bad = 0, rays = 0, pruned = 0, passed = 0, culled = 0, nobound = 0;
    const float lenses[4] = {1e-4f, 0.05f, 1e-3f, 0.5f};
    const int W = 1920, H = 1080;
    for (int ci = 0; ci < 48; ci++) {
        CamView cv;
        const double eye[3] = {3 * srand1(), 3 * srand1(), 4 * srand1()};
        if (!make_cam(cv, eye, -1.5708 + 0.5 * srand1(), 0.3 * srand1(), ci % 6 == 0, lenses[ci & 3], ci % 5 ? 35.f : 2.f))
            continue;
        for (int pi = 0; pi < 200; pi++) {
            // the axis camera's centre column and row: zero direction components
            const int x = (ci % 6 == 0 && pi < 20) ? W / 2 - 1 + (pi & 1) : (int)(urand() * (W - 1));
            const int y = (ci % 6 == 0 && pi >= 10 && pi < 30) ? H / 2 - 1 + (pi & 1) : (int)(urand() * (H - 1));
            V3 o0, d0;
            gen_ray_pixel(cv, W, H, x, y, o0, d0);
            const V3 pF = gen_ray_focal(cv, o0, d0);
            const Beam b = beam_lens(cv, pF);
            if (!b.ok) { nobound++; continue; }
            const BeamInv bi = beam_inv(b);
            // boxes and triangles near the beam's axis
            float bx[8][6];
            V3 te1[8], te2[8];
            bool miss[8], back[8];
            for (int k = 0; k < 8; k++) {
                const double t = 0.5 + 8.0 * urand(), r = k < 4 ? 0.02 : 0.5, h = 0.01 + 0.3 * urand();
                const double c[3] = {o0.x + t * d0.x + r * srand1(), o0.y + t * d0.y + r * srand1(), o0.z + t * d0.z + r * srand1()};
                for (int a = 0; a < 3; a++) { bx[k][a] = (float)(c[a] - h); bx[k][3 + a] = (float)(c[a] + h); }
                if (k == 7) bx[k][3] = bx[k][0];  // a flat box
                te1[k] = v3((float)srand1(), (float)srand1(), (float)srand1());
                te2[k] = v3((float)srand1(), (float)srand1(), (float)srand1());
                if (k & 1) {  // nearly edge-on: e2 = e1 x d + a little
                    const V3 n = cross(te1[k], d0);
                    te2[k] = v3(n.x + 1e-6f * te2[k].x, n.y + 1e-6f * te2[k].y, n.z + 1e-6f * te2[k].z);
                    te2[k] = cross(te2[k], te1[k]);
                }
                miss[k] = beam_misses_box(b, bi, bx[k][0], bx[k][1], bx[k][2], bx[k][3], bx[k][4], bx[k][5]);
                back[k] = beam_backfacing(b, te1[k], te2[k]);
                pruned += miss[k];
                culled += back[k];
            }
            for (int s = 0; s < 64; s++) {
                const Rng r{rng_key(0x5EED2026ull + ci, (uint32_t)(y * W + x), (uint32_t)s), 0u};
                V3 o, d;
                gen_ray_lens(cv, pF, r, o, d);
                rays++;
                if (!(in(b.o.x, o.x) && in(b.o.y, o.y) && in(b.o.z, o.z) && in(b.d.x, d.x) && in(b.d.y, d.y) && in(b.d.z, d.z))) {
                    bad++;
                    continue;
                }
                const V3 inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
                if (!(std::fabs(inv.x) < HUGE_VALF && std::fabs(inv.y) < HUGE_VALF && std::fabs(inv.z) < HUGE_VALF)) continue;
                if ((bi.cx && !in(bi.x, inv.x)) || (bi.cy && !in(bi.y, inv.y)) || (bi.cz && !in(bi.z, inv.z))) bad++;
                for (int k = 0; k < 8; k++) {
                    // pair_slab's arithmetic for one box
                    const float ax = (bx[k][0] - o.x) * inv.x, bxx = (bx[k][3] - o.x) * inv.x;
                    const float ay = (bx[k][1] - o.y) * inv.y, by = (bx[k][4] - o.y) * inv.y;
                    const float az = (bx[k][2] - o.z) * inv.z, bz = (bx[k][5] - o.z) * inv.z;
                    const float t0 = fmaxf(fmaxf(fminf(ax, bxx), fminf(ay, by)), fminf(az, bz));
                    const float t1 = fminf(fminf(fmaxf(ax, bxx), fmaxf(ay, by)), fmaxf(az, bz));
                    if (t0 <= t1) {
                        passed++;
                        if (miss[k]) bad++;
                    }
                    const float det = dot(te1[k], cross(d, te2[k]));
                    if (back[k] && !(det < K_EPSILON)) bad++;
                }
            }
        }
    }
    // the pinhole beam is the ray itself
    {
        const Beam b = beam_point(v3(0.f, 1.f, 2.f), v3(0.f, 0.6f, -0.8f));
        const BeamInv bi = beam_inv(b);
        if (bi.cx || !bi.cy || !bi.cz) bad++;
        if (beam_misses_box(b, bi, -1.f, 1.5f, 0.f, 1.f, 2.5f, 1.5f)) bad++;   // the ray crosses it
        if (!beam_misses_box(b, bi, -1.f, 1.5f, 3.f, 1.f, 2.5f, 4.f)) bad++;   // behind in z: entry > exit
    }
    printf("rays=%ld box_pass=%ld boxes_pruned=%ld tris_culled=%ld no_bound=%ld bad=%ld\n", rays, passed, pruned, culled,
           nobound, bad);
    return bad ? 1 : 0;
}
