"""A deterministic family of HRDI environment maps beyond the two 512x256 asset maps (DESIGN.md
section 5), shared by tests/test_env_maps_host.py and tests/test_env_maps_gpu.py.

Maps are RGBA32F arrays (H, W, 4) with fixed seeds; row 0 is the top row.  `scene_arrays` puts one into
a scene's arrays with its tables left to the device build (as test_gpu._env_only does) or taken from
the oracle's or_env_build and uploaded as given.  Everything a test asserts about what a map reaches
(guide flags, column -1, unsorted rows) is computed here from the oracle's tables and the oracle's own
upper_bound, never from the device.
"""
import ctypes as C
import functools

import numpy as np

SEED = 0x5EED2026  # the render seed default_config and the oracle's stages share
SL_LIGHT, SL_ENV_U, SL_ENV_V = 1, 2, 3  # draw slots
GUIDE_MAX = 65535  # widest / tallest table a 16-bit guide entry can index (scene_upload.cpp env_guides)
_f = C.POINTER(C.c_float)

# name -> (W, H)
SIZES = {
    "odd": (37, 13),            # non-power-of-two strides, W * H % 4 != 0
    "tiny_4x2": (4, 2),         # wrapi's i % n fallback, fewer than 16 texels in k_env_denom
    "tiny_3x3": (3, 3),
    "tiny_2x2": (2, 2),
    "tiny_1x1": (1, 1),         # rejected by the upload: (W - 1) == 0
    "wide": (2051, 5),          # more entries per row than guide bins
    "tall": (3, 1500),          # more rows than guide bins
    "bands": (96, 48),          # NaN conditional rows mid-map, marginal plateaus, column -1
    "sun_first": (64, 32),      # a CDF with one step; the seam's bilinear wrap
    "sun_last": (64, 32),
    "const": (32, 16),          # equal conditional rows
    "negative": (48, 24),       # unsorted conditional rows: guides off by k_env_check
    "zeros": (128, 64),         # NaN tables, guides off, y clamped from -1
    "w65535": (65535, 2),       # the largest guide value
    "w65536": (65536, 2),       # guides skipped by size
    "chunk_8193x1": (8193, 1),  # rejected by the upload: H == 1
    "chunk_8192x2": (8192, 2),  # k_env_denom at two full chunks
    "chunk_2731x3": (2731, 3),  # 8193 texels: k_env_denom at one chunk plus one texel
}
# Maps validate_desc refuses by design (env_w < 2 or env_h < 2): MCPT_E_INVALID
REJECTED = ("tiny_1x1", "chunk_8193x1")
REJECT_MATCH = r"mcpt error -1: HRDI env light"
ACCEPTED = tuple(n for n in SIZES if n not in REJECTED)
# The issue's expectation, checked against guides_expected() on the oracle's tables
GUIDES_OFF = ("negative", "zeros", "w65536")
SUN_ROW = 16


def _lognormal(seed, W, H, sigma=1.5):
    rng = np.random.default_rng(seed)
    t = np.zeros((H, W, 4), np.float32)
    t[..., :3] = rng.lognormal(0.0, sigma, (H, W, 3))
    return t, rng


@functools.lru_cache(maxsize=None)
def make(name):
    """The map `name` as a read-only (H, W, 4) float32 array."""
    W, H = SIZES[name]
    seed = 1000 + list(SIZES).index(name)
    if name == "odd":
        t, rng = _lognormal(seed, W, H)
        t[..., :3] *= rng.uniform(size=(H, W, 1)) > 0.2  # 20 % black texels
        t[..., 3] = rng.uniform(0.0, 9.0, (H, W))  # alpha is not the light's: the device overwrites it
    elif name == "bands":
        # Column -1 is reached through the rows below a black band (20 and 33: the marginal's plateau selects the
        # NaN row above them), row 1 and each row's first entry: about 6 % of uniform draws on average over seeds,
        # 6.6 % with this one -- clear of the 5 % the material-stage test asserts on its ~510 env samples.
        t, _ = _lognormal(2006, W, H)
        t[10:20] = 0
        t[30:33] = 0
        t[:, 40:60] = 0
    elif name in ("sun_first", "sun_last"):
        t = np.zeros((H, W, 4), np.float32)
        t[SUN_ROW, 0 if name == "sun_first" else W - 1, :3] = 1e4
    elif name == "const":
        t = np.zeros((H, W, 4), np.float32)
        t[..., :3] = 1
    elif name == "negative":
        t, rng = _lognormal(seed, W, H)
        t[..., :3] *= np.where(rng.uniform(size=(H, W, 1)) < 0.05, -1, 1)
    elif name == "zeros":
        t = np.zeros((H, W, 4), np.float32)
    elif name.startswith("tiny"):
        t = np.zeros((H, W, 4), np.float32)
        t[..., :3] = np.random.default_rng(seed).uniform(0.25, 4.0, (H, W, 3))  # positive
    else:  # wide, tall, w65535, w65536, chunk_*
        t, _ = _lognormal(seed, W, H)
    t = np.ascontiguousarray(t, np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _tables(name):
    import oracle_py

    t = oracle_py.env_build(make(name))
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def tables(name):
    """oracle.env_build of the map, computed once."""
    return _tables(name)


def with_tex(a, tex, tabs=None):
    """The scene arrays `a` under the HRDI map `tex`: tables left to the device (tabs=None), or given."""
    b = dict(a)
    b["env_mode"] = 1
    b["env_tex"] = np.ascontiguousarray(tex, np.float32)
    for k in ("marginal_y", "conds_y", "pdf"):
        b["env_" + k] = np.zeros(0, np.float32) if tabs is None else tabs[k]
    return b


def scene_arrays(a, name, given):
    """Scene arrays under map `name`.  given=False: tables built on the device at upload; True: the oracle's
    tables uploaded as given (also what the oracle itself needs)."""
    return with_tex(a, make(name), tables(name) if given else None)


def _sorted_finite(v):
    return bool(not np.isnan(v).any() and (len(v) < 2 or not (v[1:] < v[:-1]).any()))


def row_kinds(t):
    """Per conditional row of the oracle's tables: 'nan' (NaN throughout), 'sorted' (NaN-free, non-decreasing)
    or 'unsorted' (anything else), as k_env_check classifies them."""
    out = []
    for r in t["conds_y"]:
        out.append("nan" if np.isnan(r).all() else ("sorted" if _sorted_finite(r) else "unsorted"))
    return np.array(out)


def guides_expected(name):
    """Whether the upload may build search guides for the map, from the oracle's tables: both sizes within a
    16-bit guide entry, the marginal CDF sorted and NaN-free, every conditional row sorted or NaN throughout."""
    W, H = SIZES[name]
    t = tables(name)
    return bool(W <= GUIDE_MAX and H <= GUIDE_MAX and _sorted_finite(t["marginal_y"]) and
                not (row_kinds(t) == "unsorted").any())


def _ub(L, arr, val):
    return L.or_upper_bound(arr.ctypes.data_as(_f), len(arr), C.c_float(val))


def cells(oracle, t, ex, ey):
    """The reference-mode cell (x, y) env_dir samples for the draws (ex, ey), by the oracle's or_upper_bound:
    y clamped from -1 to 0, x in -1 .. W - 1 (column -1 is the reference's off-by-one)."""
    L = oracle.lib()
    my = np.ascontiguousarray(t["marginal_y"], np.float32)
    cy = np.ascontiguousarray(t["conds_y"], np.float32)
    x, y = np.zeros(len(ex), np.int64), np.zeros(len(ex), np.int64)
    for i in range(len(ex)):
        yy = max(_ub(L, my, float(ey[i])) - 1, 0)
        x[i] = _ub(L, cy[yy], float(ex[i])) - 1
        y[i] = yy
    return x, y


def material_env_draws(oracle, flags, nlights=2, seed=SEED):
    """(ex, ey, paths) of the material stage's env-light samples: path i draws with the generator keyed by
    (seed, i, sample index, length) and picks light (int)(u * nlights), 0 being the env light."""
    L = oracle.lib()
    ex, ey, ids = [], [], []
    for i, fl in enumerate(np.asarray(flags, np.uint32)):
        ln, sidx = (int(fl) >> 1) & 0xFF, int(fl) >> 13
        lid = int(np.float32(L.or_rand(seed, i, sidx, ln, SL_LIGHT)) * np.float32(nlights))
        if lid == 0 or lid == nlights:
            ex.append(L.or_rand(seed, i, sidx, ln, SL_ENV_U))
            ey.append(L.or_rand(seed, i, sidx, ln, SL_ENV_V))
            ids.append(i)
    return np.array(ex, np.float32), np.array(ey, np.float32), np.array(ids)


def uniform_draws(n=20000, seed=7):
    """n pairs of rand_float()-like draws in [0, 1): 32 random bits scaled by 2^-32 and rounded to float32, which
    can round up to 1.0 exactly as the reference's do."""
    r = np.random.default_rng(seed).integers(0, 1 << 32, (n, 2), dtype=np.uint64)
    d = (r.astype(np.float64) * 2.0 ** -32).astype(np.float32)
    return d[:, 0].copy(), d[:, 1].copy()
