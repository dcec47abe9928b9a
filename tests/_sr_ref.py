"""fp64 restatement of the super-resolution conditioning (include/vdx.h: "Cascaded super-resolution"), torch on the CPU: the box mean,
up = separable linear interpolation with half-pixel centres and clamped neighbours in its own closed form (beside
torch.nn.functional.interpolate), the augmentation, and two deliberately wrong variants the tests use to show what the bound can see."""
import torch
import torch.nn.functional as F

F64 = torch.float64

# (f, s, ft, fs): low-resolution frames and size, temporal and spatial factor -- the shapes of the GPU tests
SHAPES = [(2, 4, 2, 2), (4, 8, 1, 2), (1, 4, 4, 2), (3, 3, 2, 3), (2, 2, 1, 4), (4, 8, 1, 1)]
ODD = (3, 3, 2, 3)              # S = 9, per_sample = 486 C: the second sample's base is off 16 bytes
BIG = (8, 130, 1, 4)            # 2 163 200 outputs per sample at C = 1: past the grid cap of the elementwise launches
UP_BOUND = 1e-6                 # |kernel - fp64| for lo in [0, 1] (issue: at most 16 roundings of values <= 1)


def make_lo(B, C, f, s, seed=0):
    """A low-resolution clip [B,C,f,s,s] in [0, 1] (float32 values) that hits both ends of the range."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(B, C, f, s, s, generator=g, dtype=torch.float32)
    lo.view(-1)[0], lo.view(-1)[-1] = 0.0, 1.0
    return lo


def axis_taps(n_in, factor, mode='half_pixel'):
    """(i0, i1, w1) of every output index of one axis, in fp64: out[d] = (1 - w1) in[i0] + w1 in[i1]."""
    n_out = n_in * factor
    d = torch.arange(n_out, dtype=F64)
    if mode == 'half_pixel':                                 # src = (d + 0.5) in / out - 0.5, clamped at 0
        src = ((d + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    elif mode == 'align_corners':                            # the wrong map: corners on corners
        src = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else torch.zeros_like(d)
    elif mode == 'nearest':
        i = torch.div(torch.arange(n_out), factor, rounding_mode='floor')
        return i, i, torch.zeros(n_out, dtype=F64)
    else:
        raise ValueError(mode)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0.to(F64)


def up(lo, ft, fs, mode='half_pixel'):
    """up(2 lo - 1) in fp64 by the closed form: normalise first, then interpolate columns, rows and frames."""
    v = 2.0 * lo.to(F64) - 1.0
    for dim, factor in ((4, fs), (3, fs), (2, ft)):
        i0, i1, w1 = axis_taps(v.shape[dim], factor, mode)
        shape = [1] * 5
        shape[dim] = -1
        w1 = w1.reshape(shape)
        v = (1.0 - w1) * v.index_select(dim, i0) + w1 * v.index_select(dim, i1)
    return v


def up_interpolate(lo, ft, fs):
    """The same map through torch: F.interpolate(mode='trilinear', align_corners=False) on the normalised clip, fp64."""
    v = 2.0 * lo.to(F64) - 1.0
    return F.interpolate(v, size=(v.shape[2] * ft, v.shape[3] * fs, v.shape[4] * fs), mode='trilinear', align_corners=False)


def down(x, ft, fs):
    """Box mean of x [B,C,F,S,S] over ft x fs x fs blocks, fp64."""
    B, C, Fr, S, _ = x.shape
    return x.to(F64).reshape(B, C, Fr // ft, ft, S // fs, fs, S // fs, fs).mean(dim=(3, 5, 7))


def aug(u, z, a, b):
    """u = a_b up + b_b z per sample (a, b [B]; a = 1, b = 0 where no augmentation), fp64."""
    sh = (-1, 1, 1, 1, 1)
    return a.to(F64).reshape(sh) * u.to(F64) + b.to(F64).reshape(sh) * z.to(F64)
