"""Records which kernels libvdx launches (vdx_set_launch_hook, include/vdx.h): the names and the shape strings (template arguments +
operand shape) the launchers report, at phase 0 only and without events.  A plain module: nothing here is collected.  Tests use it to
assert the kernel a shape reaches: which form runs depends on thresholds (sequences, frames, pixels, compute units), and a retuned
threshold would otherwise move a case to another kernel without anybody noticing."""
import contextlib
import ctypes as C


class Info(C.Structure):
    _fields_ = [('kernel', C.c_char_p), ('shape', C.c_char_p), ('flops', C.c_double), ('bytes', C.c_double)]


HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(Info), C.c_void_p)


@contextlib.contextmanager
def launches():
    """with launches() as rec: ...  -> rec = [(kernel, shape), ...] in launch order; the hook is removed on exit, whatever happens."""
    from video_diffusion_nnx_amd import _lib as L
    set_hook = L._sig('vdx_set_launch_hook', None, [HOOK, C.c_void_p])
    rec = []

    def hook(user, phase, info, stream):
        if phase == 0:
            i = info.contents
            rec.append((i.kernel.decode(), i.shape.decode()))

    cb = HOOK(hook)                                   # (kept alive by this frame for as long as the library holds the pointer)
    set_hook(cb, None)
    try:
        yield rec
    finally:
        set_hook(C.cast(None, HOOK), None)


@contextlib.contextmanager
def nan_outputs():
    """with nan_outputs(): ...  -> every floating-point tensor that torch.empty hands out inside is NaN-filled.  The wrappers of
    video_diffusion_nnx_amd/ops.py allocate their outputs with torch.empty, and the caching allocator readily returns the block that
    still holds the previous run's (correct) result: with this, an element a kernel does not write is NaN, whatever was there."""
    import torch
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        return t.fill_(float('nan')) if t.is_floating_point() else t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def assert_launches(rec, expected, what=''):
    """rec: what launches() recorded; expected: [(kernel, [substrings of its shape string]), ...] -- the exact sequence of launches."""
    names = [k for k, _ in rec]
    assert names == [k for k, _ in expected], f'{what}: launched {rec}, expected {expected}'
    for (k, shape), (_, parts) in zip(rec, expected):
        for p in parts:
            assert p in shape, f'{what}: {k} ran as "{shape}", expected "{p}" in it'
