"""TEST INFRASTRUCTURE: the reference's `transforms_custom` / `transforms_elastic` (transforms.py:147-163) restated on plain torch, in any
dtype -- float64 is the truth the sampler's kernels are held to, the same code in float32 gives the bound (tf_checks.py).

kornia is not installed here, so its functions are restated LITERALLY from its documented call chains (kornia >= 0.5), normalised grids and
all -- NOT from the closed pixel-space forms the kernels implement (csrc/sampler_kornia.h), so that the two derivations check each other:

  get_rotation_matrix2d(center, angle, scale)   shift(center) @ rot(angle) @ diag(scale) @ shift(-center), rot = [[cos, sin], [-sin, cos]]
  warp_affine(src, M, dsize)                    normalize_homography -> inverse -> F.affine_grid -> F.grid_sample (bilinear, zeros,
                                                align_corners=True)
  translate(x, t)                               warp_affine with [[1, 0, tx], [0, 1, ty]]
  elastic_transform2d(x, noise, k, s, alpha)    gaussian-filtered noise * alpha added to create_meshgrid(h, w) (linspace(-1, 1)), clamped to
                                                [-1, 1], F.grid_sample (bilinear, zeros, align_corners=False)
  T.RandomErasing / F.erase                     slice assignment of the value 0 on a clone
  pad                                           F.pad(x, [4] * 4, mode='constant', value=0.5)

Pinning: unpinned against kornia itself (as `-tf fast` is against torchvision): the version note above is the contract.  The per-cut
parameters (angle, erase rectangle, jitter) come from the caller; the draws are checked separately (test_tf_host.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import reference_path as R

PAD = 4


# ---------------------------------------------------------------------------- kornia.geometry, restated
def normal_transform_pixel(height, width, dtype):
    """kornia.geometry.conversions.normal_transform_pixel: pixel coordinates -> [-1, 1] (align_corners=True convention)"""
    tr = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]], dtype=dtype)
    tr[0, 0] = tr[0, 0] * 2.0 / (width - 1.0)
    tr[1, 1] = tr[1, 1] * 2.0 / (height - 1.0)
    return tr[None]


def normalize_homography(dst_pix_trans_src_pix, dsize_src, dsize_dst):
    dtype = dst_pix_trans_src_pix.dtype
    src_norm_trans_src_pix = normal_transform_pixel(dsize_src[0], dsize_src[1], dtype)
    src_pix_trans_src_norm = torch.inverse(src_norm_trans_src_pix)
    dst_norm_trans_dst_pix = normal_transform_pixel(dsize_dst[0], dsize_dst[1], dtype)
    return dst_norm_trans_dst_pix @ (dst_pix_trans_src_pix @ src_pix_trans_src_norm)


def get_rotation_matrix2d(center, angle, scale):
    """center [B,2], angle [B] degrees, scale [B,2] -> [B,2,3]"""
    dtype, b = center.dtype, center.shape[0]
    rad = angle * (math.pi / 180.0)                         # kornia.deg2rad
    cos_a, sin_a = torch.cos(rad), torch.sin(rad)
    rot = torch.stack([cos_a, sin_a, -sin_a, cos_a], dim=-1).view(b, 2, 2)      # angle_to_rotation_matrix
    shift_m = torch.eye(3, dtype=dtype).repeat(b, 1, 1)
    shift_m[:, :2, 2] = center
    shift_m_inv = torch.eye(3, dtype=dtype).repeat(b, 1, 1)
    shift_m_inv[:, :2, 2] = -center
    scale_m = torch.eye(3, dtype=dtype).repeat(b, 1, 1)
    scale_m[:, 0, 0] = scale[:, 0]
    scale_m[:, 1, 1] = scale[:, 1]
    rotat_m = torch.eye(3, dtype=dtype).repeat(b, 1, 1)
    rotat_m[:, :2, :2] = rot
    return (shift_m @ rotat_m @ scale_m @ shift_m_inv)[:, :2, :]


def warp_affine(src, M, dsize, align_corners=True):
    b, c, h, w = src.shape
    M_3x3 = F.pad(M, [0, 0, 0, 1], 'constant', 0.0)         # convert_affinematrix_to_homography
    M_3x3[..., -1, -1] += 1.0
    dst_norm_trans_src_norm = normalize_homography(M_3x3, (h, w), dsize)
    src_norm_trans_dst_norm = torch.inverse(dst_norm_trans_src_norm)
    grid = F.affine_grid(src_norm_trans_dst_norm[:, :2, :], [b, c, dsize[0], dsize[1]], align_corners=align_corners)
    return F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=align_corners)


def translate(x, translation):
    """kornia.geometry.transform.translate: translation [B,2] = (tx, ty) pixels"""
    b = x.shape[0]
    m = torch.eye(3, dtype=x.dtype).repeat(b, 1, 1)
    m[:, 0, 2] = translation[:, 0]
    m[:, 1, 2] = translation[:, 1]
    return warp_affine(x, m[:, :2, :3], (x.shape[2], x.shape[3]), align_corners=True)


def create_meshgrid(height, width, dtype):
    xs = torch.linspace(0, width - 1, width, dtype=dtype)
    ys = torch.linspace(0, height - 1, height, dtype=dtype)
    xs = (xs / (width - 1) - 0.5) * 2
    ys = (ys / (height - 1) - 0.5) * 2
    gx, gy = torch.meshgrid(xs, ys, indexing='ij')
    return torch.stack([gx, gy], dim=-1).permute(1, 0, 2)[None]        # [1,H,W,2], last axis (x, y)


def elastic_transform2d(image, noise, align_corners=False):
    """with the ZERO noise random_elastic passes (transforms.py:23): the gaussian filter of zeros times alpha is zeros, whatever kernel
    size, sigma and alpha were drawn -- the displacement is spelled out as such"""
    b, c, h, w = image.shape
    disp = torch.cat([noise[:, :1] * 0.0, noise[:, 1:] * 0.0], dim=1).permute(0, 2, 3, 1)
    grid = create_meshgrid(h, w, image.dtype)
    return F.grid_sample(image, (grid + disp).clamp(-1, 1), mode='bilinear', padding_mode='zeros', align_corners=align_corners)


# ---------------------------------------------------------------------------- the closures of transforms.py
def random_rotate(image_t, alpha):
    """transforms.py:53-71 with the drawn angle `alpha` (degrees)"""
    b, _, h, w = image_t.shape
    angle = torch.ones(b, dtype=image_t.dtype) * alpha
    scale = torch.ones(b, 2, dtype=image_t.dtype)
    center = torch.ones(b, 2, dtype=image_t.dtype)
    center[..., 0] = (image_t.shape[3] - 1) / 2
    center[..., 1] = (image_t.shape[2] - 1) / 2
    M = get_rotation_matrix2d(center, angle, scale)
    return warp_affine(image_t, M, dsize=(h, w))


def chain(cut, prm, elastic, normalise=True):
    """cut [1,3,n,n] -> [1,3,n+8,n+8]; prm: dict(angle=degrees, erase=(i,j,h,w) on the padded canvas or None, shift=(dx,dy))"""
    x = F.pad(cut, [PAD] * 4, mode='constant', value=0.5)                      # transforms.py:148,157
    if elastic and prm.get('erase') is not None:                               # T.RandomErasing(0.2), value 0
        i, j, h, w = prm['erase']
        x = x.clone()
        x[..., i:i + h, j:j + w] = 0.0
    x = random_rotate(x, float(prm['angle']))                                  # transforms.py:150,160
    if elastic:                                                                # transforms.py:17-25
        x = elastic_transform2d(x, torch.zeros(1, 2, x.shape[2], x.shape[3], dtype=x.dtype))
    dx, dy = prm['shift']
    x = translate(x, torch.tensor([[dx, dy]], dtype=x.dtype))                  # transforms.py:27-33
    return R.normalize(x) if normalise else x


def per_cut(prms, elastic, normalise=True, window=None):
    """-> per_cut(c, cut) for oracle.reference_path.slice_imgs / ReferenceRun; window = n: the top-left n x n the ViT's conv reads"""
    def f(c, cut):
        y = chain(cut, prms[c], elastic, normalise)
        return y if window is None else y[:, :, :window, :window]
    return f
