"""TEST INFRASTRUCTURE: the crop sampler (utils.py:243-253) and the `-tf fast` chain (transforms.py:165-170) restated COORDINATE-EXACT in
float64 -- the truth the kernels of csrc/sampler_crop.h, sampler_crop_adjoint.h and sampler_warp.h are held to (sampler_checks.py).

A plain float64 run of the oracle is no truth for these kernels: the float32 SOURCE COORDINATES are part of the operation's definition (ATen
computes them in float32, the kernels copy that on purpose), and moving them to float64 moves the result by 1e-5 .. 5e-4 -- as far as the
kernels are from it.  So here the coordinates are float32, in ATen's / torchvision's operation order, and everything after them is float64:

  crop + resize   F.interpolate(bicubic, align_corners=True): scale = (cs - 1) / (size - 1), src = scale * i, floor, t = src - floor in
                  float32 (scale = 0 when size == 1); the four cubic-convolution weights (A = -0.75) from t in float64; taps clamped into
                  [0, cs - 1] and accumulated into the explicit matrix M[size, cs] per cut and axis.  Forward M_y . crop . M_x^T, adjoint the
                  transposed products summed over the cuts into the padded frame; overscan / overmax fold that frame back onto the image
                  through oracle.reference_path.tile_pad_index.
  -tf fast        RandomPerspective -> RandomErasing -> rotation, torchvision's tensor path: the normalised grid (_perspective_grid,
                  _gen_affine_grid) and its unnormalisation ((g + 1) n - 1) / 2 in float32, in the order of the operations; the bilinear
                  weights, the ones-mask (the sum of the in-range weights), the erase and the sums in float64.  Every stage is an explicit
                  sparse linear map (Sparse), so the adjoint is the exact transpose of the forward by construction.

Nothing here is shared with the kernels or with the float32 oracle (oracle/reference_path.py, oracle/augment_ref.py) beyond the wrap index
and the cubic polynomial; test_emu_sampler.py pins it against the reference-generated golden and against the float32 oracle before it judges
a kernel.  rounding_bound() is the a-priori float32 error of the oracle that those pins assert."""
import math

import numpy as np

from oracle import reference_path as R

F32 = np.float32
EPS32 = 2.0 ** -24
MEAN = np.array(R.CLIP_MEAN, dtype=np.float64).reshape(3, 1, 1)
STD = np.array(R.CLIP_STD, dtype=np.float64).reshape(3, 1, 1)


# ---------------------------------------------------------------------------- crop + bicubic resize
def axis_matrix(cs, size, taps=False):
    """[size, cs] float64: one axis of F.interpolate(cut of cs pixels -> size, bicubic, align_corners=True); taps: how many of the four taps
    of an output land on each source position instead of their weights"""
    scale = F32(cs - 1) / F32(size - 1) if size > 1 else F32(0)
    src = (scale * np.arange(size, dtype=F32)).astype(F32)
    x0 = np.floor(src)
    t = (src - x0).astype(F32).astype(np.float64)
    w = R.cubic_coeffs(t)                                   # taps -1, 0, +1, +2, float64
    M = np.zeros((size, cs), dtype=np.float64)
    rows = np.arange(size)
    for k in range(4):
        np.add.at(M, (rows, np.clip(x0.astype(np.int64) - 1 + k, 0, cs - 1)), 1.0 if taps else w[k])
    return M


class Sparse:
    """a linear map [.., n_in] -> [.., n_out] as (row, column, value) triplets"""

    def __init__(self, n_out, n_in, rows, cols, vals):
        self.n_out, self.n_in, self.rows, self.cols, self.vals = n_out, n_in, rows, cols, vals

    def fwd(self, x):
        return np.stack([np.bincount(self.rows, weights=self.vals * c[self.cols], minlength=self.n_out) for c in x])

    def adj(self, y):
        return np.stack([np.bincount(self.cols, weights=self.vals * c[self.rows], minlength=self.n_in) for c in y])

    def absolute(self):
        return Sparse(self.n_out, self.n_in, self.rows, self.cols, np.abs(self.vals))

    def ones(self):
        return Sparse(self.n_out, self.n_in, self.rows, self.cols, np.ones_like(self.vals))


# ---------------------------------------------------------------------------- the warps of -tf fast
def perspective_grid(coeffs, n):
    """torchvision _perspective_grid -> float32 source pixel coordinates (ix, iy) of every output pixel, row-major"""
    a = np.asarray(coeffs, dtype=F32)
    hn = F32(0.5) * F32(n)
    i, j = np.divmod(np.arange(n * n), n)
    x, y = j.astype(F32) + F32(0.5), i.astype(F32) + F32(0.5)
    g1x = x * (a[0] / hn) + y * (a[1] / hn) + (a[2] / hn)
    g1y = x * (a[3] / hn) + y * (a[4] / hn) + (a[5] / hn)
    g2 = x * a[6] + y * a[7] + F32(1)
    return _unnormalise(g1x / g2 - F32(1), n), _unnormalise(g1y / g2 - F32(1), n)


def rotation_grid(angle, n):
    """torchvision _gen_affine_grid with the inverse rotation matrix [cos, sin, 0; -sin, cos, 0] (degrees) -> float32 (ix, iy)"""
    rot = math.radians(float(angle))
    cs, sn = F32(math.cos(rot)), F32(math.sin(rot))
    hn = F32(0.5) * F32(n)
    i, j = np.divmod(np.arange(n * n), n)
    x, y = -F32(n) * F32(0.5) + F32(0.5) + j.astype(F32), -F32(n) * F32(0.5) + F32(0.5) + i.astype(F32)
    gx = x * (cs / hn) + y * (sn / hn) + (F32(0) / hn)
    gy = x * (-sn / hn) + y * (cs / hn) + (F32(0) / hn)
    return _unnormalise(gx, n), _unnormalise(gy, n)


def _unnormalise(g, n):
    """at::native grid_sampler_unnormalize, align_corners=False, float32"""
    assert g.dtype == F32
    return ((g + F32(1)) * F32(n) - F32(1)) * F32(0.5)


def bilinear_map(ix, iy, n):
    """grid_sample(bilinear, zeros) of the image and of a ones-mask, multiplied (torchvision's fill = 0): out[p] = m[p] sum_k w_k[p] src[tap_k],
    m = the sum of the in-range weights; weights float64 from the float32 coordinates"""
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    fx, fy = ix.astype(np.float64) - x0, iy.astype(np.float64) - y0
    p = np.arange(n * n)
    taps, mask = [], np.zeros(n * n)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            w = (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)
            ok = (xx >= 0) & (xx < n) & (yy >= 0) & (yy < n)
            mask += np.where(ok, w, 0.0)
            taps.append((p[ok], (yy * n + xx)[ok], w[ok]))
    rows, cols = np.concatenate([t[0] for t in taps]), np.concatenate([t[1] for t in taps])
    return Sparse(n * n, n * n, rows, cols, np.concatenate([t[2] for t in taps]) * mask[rows])


def erase_map(rect, n):
    """F.erase: img[..., i:i + h, j:j + w] = 0"""
    i, j, h, w = (int(v) for v in rect)
    keep = np.ones((n, n), dtype=bool)
    keep[i:i + h, j:j + w] = False
    p = np.nonzero(keep.reshape(-1))[0]
    return Sparse(n * n, n * n, p, p, np.ones(p.size))


def chain_maps(prm, n):
    """the stages of transforms_fast for one cut, in order, as (map, is a warp); angle None = no rotation stage, 0.0 = the identity resample
    torchvision still performs"""
    out = []
    if prm.get('persp') is not None:
        out.append((bilinear_map(*perspective_grid(prm['persp'], n), n), True))
    if prm.get('erase') is not None:
        out.append((erase_map(prm['erase'], n), False))
    if prm.get('angle') is not None:
        out.append((bilinear_map(*rotation_grid(prm['angle'], n), n), True))
    return out


# ---------------------------------------------------------------------------- the whole sampler
class Sampler:
    """slice_imgs of an H x W image with an explicit crop table ([S,3] rows (csize, offx, offy) in the padded frame), optionally followed
    per cut by the -tf fast chain with explicit parameters (dicts persp / erase / angle)"""

    def __init__(self, H, W, table, size, align='uniform', prms=None):
        self.H, self.W, self.size, self.S = H, W, size, len(table)
        self.table = [tuple(int(v) for v in row) for row in table]
        self.Hp, self.Wp = R.padded_size(H, W, align) if 'over' in align else (H, W)
        py0, px0 = (self.Hp - H) // 2, (self.Wp - W) // 2
        self.yy, self.xx = R.tile_pad_index(H, py0, self.Hp - H - py0), R.tile_pad_index(W, px0, self.Wp - W - px0)
        mats = {}
        for cs, _, _ in self.table:
            if cs not in mats:
                mats[cs] = (axis_matrix(cs, size), axis_matrix(cs, size, taps=True))
        self.M = [mats[cs][0] for cs, _, _ in self.table]
        # mode 'abs': |w| + 1/4 on every tap (rounding_bound: the absolute float32 error of a cubic weight, in units of gamma)
        self.Mabs = [np.abs(mats[cs][0]) + 0.25 * mats[cs][1] for cs, _, _ in self.table]
        self.chains = [chain_maps(p, size) for p in prms] if prms is not None else [[] for _ in self.table]

    # stage modes: 'exact'; 'abs' = the absolute values of every weight; for one warp stage `ones_at`: unit weights on its taps
    def _stage(self, m, warp, mode, hit):
        return m.ones() if hit else (m.absolute() if mode == 'abs' else m)

    def forward(self, img, mode='exact', ones_at=None):
        """img [3,H,W] float64 -> raw cuts [S,3,size,size]"""
        n = self.size
        pad = img[:, self.yy][:, :, self.xx]
        out = np.empty((self.S, 3, n, n))
        for s, (cs, ox, oy) in enumerate(self.table):
            M = self.Mabs[s] if mode == 'abs' else self.M[s]
            v = (M @ pad[:, oy:oy + cs, ox:ox + cs] @ M.T).reshape(3, n * n)
            k = 0
            for m, warp in self.chains[s]:
                v = self._stage(m, warp, mode, warp and ones_at == k).fwd(v)
                k += warp
            out[s] = v.reshape(3, n, n)
        return out

    def adjoint(self, g, mode='exact', ones_at=None):
        """g [S,3,size,size] float64 = the gradient of the raw cuts -> the gradient of the image [3,H,W]"""
        n = self.size
        dpad = np.zeros((3, self.Hp, self.Wp))
        for s, (cs, ox, oy) in enumerate(self.table):
            M = self.Mabs[s] if mode == 'abs' else self.M[s]
            v = g[s].reshape(3, n * n)
            k = sum(w for _, w in self.chains[s])
            for m, warp in reversed(self.chains[s]):
                k -= warp
                v = self._stage(m, warp, mode, warp and ones_at == k).adj(v)
            dpad[:, oy:oy + cs, ox:ox + cs] += M.T @ v.reshape(3, n, n) @ M
        dimg = np.zeros((3, self.H, self.W))
        np.add.at(dimg, (slice(None), self.yy[:, None], self.xx[None, :]), dpad)
        return dimg

    def warp_stages(self):
        return max([sum(w for _, w in c) for c in self.chains] + [0])


def normalise(raw):
    return (raw - MEAN) / STD


def normalise_adjoint(g):
    return g / STD


# ---------------------------------------------------------------------------- the float32 oracle's a-priori error
def rounding_bound(sampler, x, adjoint):
    """Element-wise bound on |float32 oracle - this restatement| for sampler.forward(x) / sampler.adjoint(x), from the arithmetic alone:

      gamma |A| |x|       the float32 roundings of one term's weight (a bilinear weight and the mask: 8 operations; the cubic polynomial: 9, on
                          intermediates that reach 6 whatever the weight, an ABSOLUTE 16 2^-24 = gamma / 4 per weight, which |A| carries as
                          |w| + 1/4 on every tap) and of the sums: a cut's 16 taps, two 4-tap warps, and in the adjoint one accumulation per cut on top, each a
                          relative 2^-24 of the sum of the absolute terms: gamma = (64 + S [adjoint]) 2^-24
      10 delta Ones_k     per warp stage k: the oracle's normalised grid comes out of a float32 matrix product whose summation order and
                          contraction are the BLAS's, so its source coordinate may differ from the restatement's by delta = 12 n 2^-24
                          pixels (the grid, of magnitude <= 2 after the perspective division, carries <= 8 roundings, the unnormalisation
                          scales them by n / 2 and adds 3 of magnitude n).  A tap weight (a product of two factors <= 1) moves by <= 2 delta,
                          the mask by <= 8 delta: <= 10 delta times the unit-weight footprint, pushed through the absolute maps around it."""
    run = sampler.adjoint if adjoint else sampler.forward
    gamma = (64 + (sampler.S if adjoint else 0)) * EPS32
    bound = gamma * run(np.abs(x), mode='abs')
    delta = 12 * sampler.size * EPS32
    for k in range(sampler.warp_stages()):
        bound = bound + 10 * delta * run(np.abs(x), mode='abs', ones_at=k)
    return bound
