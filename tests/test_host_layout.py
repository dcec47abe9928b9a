"""CPU tests: libvdx.so loads without a GPU, exports every symbol include/vdx.h declares, and its parameter
layout agrees (names, shapes, order) with the oracle's independent restatement of the reference tree."""
import os
import re

import numpy as np
import pytest

from oracle import unet3d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from video_diffusion_nnx_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'vdx.h')).read()
    names = set(re.findall(r'\b(vdx_[a-z0-9_]+)\s*\(', hdr))
    assert len(names) >= 20
    # the test-facing forward forms ("Forward forms of the network") are part of what the header declares
    assert {'vdx_attention_heads_forward', 'vdx_attention_long_forward', 'vdx_sla_heads_forward', 'vdx_resblock_tail_ex',
            'vdx_resblock_tail_rc_head_bf16', 'vdx_final_conv_ex', 'vdx_init_conv_ex', 'vdx_resblock_scale_shift',
            'vdx_attention_heads_scratch_bytes', 'vdx_attention_long_scratch_bytes'} <= names
    for n in sorted(names):
        assert hasattr(_lib.lib, n), f'libvdx.so does not export {n}'
    assert _lib.vdx_version() >= 1


@pytest.mark.parametrize('kw', [dict(dim=64, channels=1), dict(dim=32, channels=1), dict(dim=16, channels=3, cond_dim=32),
                                dict(dim=16, channels=3, use_bert_text_cond=True), dict(dim=24, channels=2, dim_mults=(1, 2)),
                                dict(dim=16, channels=3, use_sparse_linear_attn=False)])
def test_param_layout_matches_oracle_spec(kw):
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(rngs=0, device='cpu', **kw)
    spec = R.param_spec(R.UnetConfig(**kw))
    assert [(n, tuple(s)) for n, s, _ in m.param_table] == [(n, tuple(s)) for n, s in spec]
    offs = [o for _, _, o in m.param_table]
    assert all(o % 4 == 0 for o in offs) and offs == sorted(offs)
    sd = m.state_dict()
    assert sum(v.numel() for v in sd.values()) == sum(int(np.prod(s)) for _, s in spec)


def test_default_init_statistics():
    from video_diffusion_nnx_amd.unet3d import Unet3D
    m = Unet3D(dim=32, rngs=3, channels=1, device='cpu')
    sd = m.state_dict()
    k = sd['downs.1.0.block_1.proj.kernel']
    assert abs(k.std().item() - (1.0 / (9 * 32)) ** 0.5) < 0.1 * (1.0 / (9 * 32)) ** 0.5
    assert sd['downs.0.0.block_1.proj.bias'].abs().max() == 0 and (sd['downs.0.0.block_1.norm.scale'] == 1).all()
    m2 = Unet3D(dim=32, rngs=3, channels=1, device='cpu')
    assert (m2.flat_params == m.flat_params).all()           # deterministic in the seed


def test_no_gpu_means_loud_failure():
    import torch
    from video_diffusion_nnx_amd.unet3d import Unet3D
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    m = Unet3D(dim=16, rngs=0, channels=3, device='cpu')
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 4, 16, 16), torch.zeros(1, dtype=torch.long))


def test_bad_config_is_rejected():
    from video_diffusion_nnx_amd import _lib
    from video_diffusion_nnx_amd.unet3d import Unet3D
    with pytest.raises(_lib.VdxError):
        Unet3D(dim=20, rngs=0, device='cpu')                 # not a multiple of 8
