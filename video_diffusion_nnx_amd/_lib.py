"""ctypes binding of libvdx.so (the C ABI declared in include/vdx.h).

The library is loaded here and nowhere else; the modules that call an entry bind it with `_sig` (here, or next to its caller:
gaussian_diffusion.py, train_step.py, ops.py, unet3d.py, timestep_sampler.py).  There is NO fallback: if the shared library is
missing or a symbol cannot be resolved, importing the binding module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VDX_LIB: a variant build of the same sources (tools/ab_variants.sh: A/B timing of kernel changes); the product path is the in-tree library
LIB_PATH = os.environ.get('VDX_LIB') or os.path.join(_HERE, 'libvdx.so')

MODE_F32 = 0
MODE_BF16 = 1
MODE_F16 = 2
MODES = {'f32': MODE_F32, 'fp32': MODE_F32, 'float32': MODE_F32, 'bf16': MODE_BF16, 'bfloat16': MODE_BF16,
         'f16': MODE_F16, 'fp16': MODE_F16, 'float16': MODE_F16}
GN_SLOTS = 32


class VdxError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f'{LIB_PATH} not found: the HIP extension is required (no CPU fallback exists). '
        'Build it with `python -c "import __graft_entry__ as g; g.build()"` or `make -C video_diffusion_nnx_amd/csrc`.')

lib = C.CDLL(LIB_PATH)

c_void_p, c_int, c_size_t, c_float, c_double = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double


class ConvDesc(C.Structure):
    _fields_ = [
        ('x0', c_void_p), ('x1', c_void_p), ('c0', c_int), ('c1', c_int),
        ('packed_w', c_void_p), ('bias', c_void_p), ('y', c_void_p), ('cout', c_int),
        ('batch', c_int), ('frames', c_int), ('h', c_int), ('w', c_int),
        ('kind', c_int), ('kh', c_int), ('kw', c_int), ('stride', c_int),
        ('in_stats', c_void_p), ('gamma', c_void_p), ('beta', c_void_p), ('groups', c_int),
        ('scale_shift', c_void_p), ('scale_shift_stride', c_int),
        ('out_stats', c_void_p), ('out_groups', c_int),
        ('x_bf16', c_int), ('y_bf16', c_int),
        ('res', c_void_p), ('res_bf16', c_int),
    ]


def _sig(name, restype, argtypes):
    fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


vdx_last_error = _sig('vdx_last_error', C.c_char_p, [])
vdx_version = _sig('vdx_version', c_int, [])
vdx_packed_conv_bytes = _sig('vdx_packed_conv_bytes', c_size_t, [c_int, c_int, c_int, c_int])
vdx_pack_conv_weights = _sig('vdx_pack_conv_weights', c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p])
vdx_gn_stats_bytes = _sig('vdx_gn_stats_bytes', c_size_t, [c_int, c_int])
vdx_conv_forward = _sig('vdx_conv_forward', c_int, [c_int, C.POINTER(ConvDesc), c_void_p])


def check(status: int) -> None:
    if status != 0:
        raise VdxError(f'libvdx status {status}: {vdx_last_error().decode()}')


def ptr(t) -> int:
    """Device pointer of a torch tensor (must be contiguous) or 0 for None."""
    if t is None:
        return 0
    assert t.is_contiguous(), 'libvdx needs contiguous tensors'
    return t.data_ptr()


def stream_ptr() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream

c_long = C.c_long
vdx_resblock_tail = _sig('vdx_resblock_tail', c_int, [c_void_p] * 6 + [c_int, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p])
vdx_gn_silu_apply_bf16 = _sig('vdx_gn_silu_apply_bf16', c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_int, c_long, c_void_p])
vdx_resblock_tail_rc_bf16 = _sig('vdx_resblock_tail_rc_bf16', c_int, [c_void_p] * 3 + [c_int, c_int] + [c_void_p] * 6 + [c_int, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p])
vdx_init_conv = _sig('vdx_init_conv', c_int, [c_void_p] * 4 + [c_int] * 7 + [c_void_p])
vdx_final_conv = _sig('vdx_final_conv', c_int, [c_void_p] * 4 + [c_long, c_int, c_int, c_void_p])
vdx_time_mlp = _sig('vdx_time_mlp', c_int, [c_void_p] * 5 + [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p])
vdx_attention_forward = _sig('vdx_attention_forward', c_int, [c_int] + [c_void_p] * 6 + [c_int] * 7 + [c_void_p])
vdx_attention_forward_ex = _sig('vdx_attention_forward_ex', c_int, [c_int] + [c_void_p] * 6 + [c_int] * 8 + [c_void_p])
vdx_attention_forward_bf16 = _sig('vdx_attention_forward_bf16', c_int, [c_void_p] * 6 + [c_int] * 8 + [c_void_p])
vdx_sla_forward_bf16 = _sig('vdx_sla_forward_bf16', c_int, [c_void_p] * 7 + [c_int] * 6 + [c_void_p])
vdx_sla_workspace_bytes = _sig('vdx_sla_workspace_bytes', c_size_t, [c_int] * 4)
vdx_sla_forward = _sig('vdx_sla_forward', c_int, [c_int] + [c_void_p] * 7 + [c_int] * 6 + [c_void_p])


# forward forms of the network (vdx.h: "Forward forms of the network (test-facing)")
class SsLayer(C.Structure):
    _fields_ = [('w_off', c_long), ('b_off', c_long), ('g_off', c_long), ('be_off', c_long), ('out_off', c_long), ('n', c_int), ('pad_', c_int)]


vdx_attention_heads_scratch_bytes = _sig('vdx_attention_heads_scratch_bytes', c_size_t, [c_int] * 4)
vdx_attention_long_scratch_bytes = _sig('vdx_attention_long_scratch_bytes', c_size_t, [c_int] * 5)
vdx_attention_heads_forward = _sig('vdx_attention_heads_forward', c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 5 + [c_size_t] + [c_int] * 7 + [c_void_p])
vdx_attention_long_forward = _sig('vdx_attention_long_forward', c_int, [c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 5 + [c_size_t] + [c_int] * 6 + [c_void_p])
vdx_sla_heads_forward = _sig('vdx_sla_heads_forward', c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 5 + [c_size_t] + [c_int] * 5 + [c_void_p])
vdx_resblock_tail_ex = _sig('vdx_resblock_tail_ex', c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                            c_int, c_int, c_long, c_void_p])
vdx_resblock_tail_rc_head_bf16 = _sig('vdx_resblock_tail_rc_head_bf16', c_int, [c_void_p] * 3 + [c_int, c_int] + [c_void_p] * 5 + [c_int, c_void_p, c_void_p, c_int] +
                                      [c_void_p] * 3 + [c_int, c_long, c_void_p])
vdx_final_conv_ex = _sig('vdx_final_conv_ex', c_int, [c_void_p, c_int] + [c_void_p] * 3 + [c_long, c_int, c_int, c_void_p])
vdx_init_conv_ex = _sig('vdx_init_conv_ex', c_int, [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p])
vdx_resblock_scale_shift = _sig('vdx_resblock_scale_shift', c_int, [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p])

# classifier-free guidance (vdx.h: "Classifier-free guidance"): the combine kernel and the three guided loops
_u64 = C.c_uint64
vdx_cfg_scratch_doubles = _sig('vdx_cfg_scratch_doubles', c_size_t, [c_int])
vdx_cfg_combine = _sig('vdx_cfg_combine', c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p, c_int, c_long, c_void_p])
vdx_p_sample_loop_guided = _sig('vdx_p_sample_loop_guided', c_int, [c_void_p] * 8 + [c_int, c_int, c_void_p, _u64, c_int, c_float, c_void_p, c_float, c_float,
                                                                    c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p])
vdx_ddim_sample_loop_guided = _sig('vdx_ddim_sample_loop_guided', c_int, [c_void_p] * 9 + [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_float,
                                                                          c_float, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p])
vdx_dpm_sample_loop_guided = _sig('vdx_dpm_sample_loop_guided', c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_void_p,
                                                                        c_float, c_float, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p])

# held-out evaluation (vdx.h: "Held-out evaluation"): the captured loop; the single-step entries are bound in ops.py
VLB_ROWS = 9                                     # VDX_VLB_ROWS: the rows of the table of doubles (gaussian_diffusion.make_vlb_tables)
vdx_vlb_scratch_doubles = _sig('vdx_vlb_scratch_doubles', c_size_t, [c_int])
vdx_vlb_loop = _sig('vdx_vlb_loop', c_int, [c_void_p] * 9 + [c_int, c_void_p, c_int, c_int, c_void_p, _u64, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                            c_int, c_int, c_void_p])

# learned variances (vdx.h: "Learned variances"): the step, the captured sampling loop, the hybrid loss and the bound with the model's variance
LV_ROWS = 9                                      # VDX_LV_ROWS: the rows of the table of doubles (gaussian_diffusion.make_lv_tables)
vdx_p_sample_step_lv = _sig('vdx_p_sample_step_lv', c_int, [c_void_p] * 5 + [c_int, _u64, c_void_p, c_void_p, _u64, _u64, c_void_p, c_int, c_float, c_float,
                                                            c_int, c_int, c_long, c_void_p])
vdx_p_sample_loop_lv = _sig('vdx_p_sample_loop_lv', c_int, [c_void_p] * 9 + [c_int, c_int, c_int, c_void_p, _u64, c_int, c_float, c_float, c_void_p, c_size_t,
                                                            c_int, c_int, c_void_p])
vdx_hybrid_scratch_doubles = _sig('vdx_hybrid_scratch_doubles', c_size_t, [c_int])
vdx_hybrid_loss = _sig('vdx_hybrid_loss', c_int, [c_void_p] * 5 + [c_int, c_float, c_float, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_int, c_int, c_long, c_void_p])
# (vdx.h: "Loss-aware timestep sampling": vdx_hybrid_loss with importance weights; the sampler's own entries are bound in timestep_sampler.py)
vdx_hybrid_loss_w = _sig('vdx_hybrid_loss_w', c_int, [c_void_p] * 5 + [c_int, c_float, c_float, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p,
                                                      c_int, c_int, c_long, c_void_p, c_void_p])
vdx_vlb_terms_lv = _sig('vdx_vlb_terms_lv', c_int, [c_void_p] * 4 + [c_int, c_void_p, _u64, _u64, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p])
vdx_vlb_loop_lv = _sig('vdx_vlb_loop_lv', c_int, [c_void_p] * 9 + [c_int, c_void_p, c_int, c_int, c_void_p, _u64, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                                  c_int, c_int, c_void_p])
vdx_final_conv_backward_wide = _sig('vdx_final_conv_backward_wide', c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_long, c_int, c_int, c_void_p, c_size_t, c_void_p])

# cascaded super-resolution (vdx.h: "Cascaded super-resolution"): the kernels around xin = [ x_t | u ] and the three loops over it
DRAW_LOWRES = 1 << 61                            # VDX_DRAW_LOWRES: the augmentation draw of the sampling chains
vdx_lowres_down = _sig('vdx_lowres_down', c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p])
vdx_lowres_input = _sig('vdx_lowres_input', c_int, [c_void_p] * 8 + [c_int, _u64, _u64, c_float, c_float] + [c_int] * 6 + [c_void_p])
vdx_lowres_pack = _sig('vdx_lowres_pack', c_int, [c_void_p, c_void_p, c_int, c_long, c_void_p])
vdx_p_sample_loop_sr = _sig('vdx_p_sample_loop_sr', c_int, [c_void_p] * 9 + [c_int, c_int, c_void_p, _u64, c_int, c_float, c_void_p, c_void_p, c_size_t,
                                                            c_int, c_int, c_void_p])
vdx_ddim_sample_loop_sr = _sig('vdx_ddim_sample_loop_sr', c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                                                  c_size_t, c_int, c_int, c_void_p])
vdx_dpm_sample_loop_sr = _sig('vdx_dpm_sample_loop_sr', c_int, [c_void_p] * 11 + [c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                                                c_size_t, c_int, c_int, c_void_p])

# mixed noise (vdx.h: "Mixed noise"): the generator, the ancestral step that draws it in the kernel, and the loop over that step
# (vdx_p_sample_loop_guided's arguments with a, b after the cfg scratch)
DRAW_SHARED = 1 << 60                            # VDX_DRAW_SHARED: the shared component of draw d is draw DRAW_SHARED + d
vdx_randn_mixed = _sig('vdx_randn_mixed', c_int, [c_void_p, c_int, c_int, c_int, c_long, c_float, c_float, _u64, _u64, c_void_p, c_void_p])
vdx_p_sample_step_mixed = _sig('vdx_p_sample_step_mixed', c_int, [c_void_p] * 5 + [c_int, c_int, c_float, c_float, _u64, _u64, c_void_p, c_void_p, c_int, c_int,
                                                                  c_int, c_long, c_void_p])
vdx_p_sample_loop_mixed = _sig('vdx_p_sample_loop_mixed', c_int, [c_void_p] * 8 + [c_int, c_int, c_void_p, _u64, c_int, c_float, c_void_p, c_float, c_float,
                                                                  c_void_p, c_float, c_float, c_void_p, c_size_t, c_int, c_int, c_void_p])

# v-prediction (vdx.h: "v-prediction"): the conversion behind the forward, the weighted loss pass and the handle's prediction state
vdx_v_to_eps = _sig('vdx_v_to_eps', c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_long, c_void_p])
vdx_v_loss_scratch_doubles = _sig('vdx_v_loss_scratch_doubles', c_size_t, [c_int])
vdx_v_loss = _sig('vdx_v_loss', c_int, [c_void_p] * 8 + [c_int, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p])
vdx_set_prediction = _sig('vdx_set_prediction', c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int])
vdx_get_prediction = _sig('vdx_get_prediction', c_int, [c_void_p])

# self-conditioning (vdx.h: "Self-conditioning"): the x0 estimate behind the forward and the handle's self-condition state
vdx_selfcond_x0 = _sig('vdx_selfcond_x0', c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_long,
                                                  c_void_p])
vdx_set_self_condition = _sig('vdx_set_self_condition', c_int, [c_void_p, c_int, c_void_p, c_int])
vdx_get_self_condition = _sig('vdx_get_self_condition', c_int, [c_void_p])
