"""Launch chains of the reverse pass on the GPU.  Without a device tests/test_host_bwd_routes.py sees the first launch of a chain only; here
the whole sequence each launcher reports (tests/_launch_hook.py) is pinned at the smallest shapes that tell the chains apart, through the
wrappers of video_diffusion_nnx_amd/ops.py on real tensors: the weight gradient with and without room for its slots, the split q|k|v
form, the three passes of the norm backward, both passes of the three SLA forms, the head, the time-MLP backward per stage and for the
whole table, and the two slot-sum kernels.  Every case also runs without the hook and compares the outputs bit for bit: a report must
not change a result.  Values are covered elsewhere (test_gpu_backward_forms.py, test_gpu_conv_backward.py, test_gpu_step_kernels.py)."""
import pytest
import torch

from _launch_hook import assert_launches, launches

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, BF = torch.float32, torch.bfloat16


def _ints(*shape, seed=0, lo=-2, hi=3, dtype=F32):
    """small integers: every sum of products below is exact in bf16 operands and fp32 accumulators, in any order of addition, so the
    float-atomics form gives the same bits on every run and the same bits as the slot form"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(dtype).to(DEV)


def _randn(*shape, seed=0, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _flat(out):
    if isinstance(out, dict):
        out = list(out.values())
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out if o is not None for t in _flat(o)]


def _hooked_and_plain(fn):
    """fn() under the hook and without it -> (launches, outputs); the outputs must be equal bit for bit"""
    with launches() as rec:
        got = _flat(fn())
        torch.cuda.synchronize()
    plain = _flat(fn())
    torch.cuda.synchronize()
    assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain))
    assert all(torch.isfinite(t.float()).all() for t in got)
    return rec, got


def test_weight_gradient_with_and_without_room_for_its_slots():
    from video_diffusion_nnx_amd import ops
    x, dy = _ints(1, 2, 16, 16, 64, seed=1), _ints(1, 2, 16, 16, 64, seed=2)
    need = 4 * (9 * 64 * 64 + 64)                            # 8 x 16 patches: 2 frames x 2 x 1 chunks of a dW tile + a bias row
    main = ('conv_wgrad16_kernel', ['<NT 9, NG 2, PF 1, X16 0, DY16 0>', 'conv3x3 64->64 2x16x16', '+db', 'patch 8x16 chunks4'])
    outs = {}
    for floats, det in ((need, 1), (need - 1, 0)):
        scratch = torch.empty(floats, dtype=F32, device=DEV)
        rec, outs[det] = _hooked_and_plain(lambda: ops.conv_backward_weights_ex(x, dy, (1, 3, 3, 64, 64), bias=True, scratch=scratch))
        chain = [(main[0], main[1] + [f'det {det}'])]
        if det:
            chain += [('slot_sum_kernel', [f'slots4 E{9 * 64 * 64} Cout64 split0']), ('slot_sum_kernel', ['slots4 E64 Cout64 split0'])]
        assert_launches(rec, chain, f'3x3 weight gradient, det {det}')
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[0]))      # (exact sums: slots and atomics agree to the bit)
    assert outs[1][0].abs().max() > 0 and outs[1][1].abs().max() > 0


def test_split_qkv_weight_gradient():
    from video_diffusion_nnx_amd import ops
    x, dqkv = _ints(1, 2, 4, 4, 64, seed=3), _ints(1, 2, 4, 4, 768, seed=4)
    scratch = torch.empty(1 << 16, dtype=F32, device=DEV)
    rec, out = _hooked_and_plain(lambda: ops.conv_backward_weights_ex(x, dqkv, (1, 64, 768), k=1, split=256, bias=True, scratch=scratch))
    assert_launches(rec, [('wgrad1x1_kernel', ['<X16 0, DY16 0, NCO 4>', 'conv1x1 64->768 rows32 split256 slots1 det 1']),
                          ('slot_sum_kernel', [f'slots1 E{64 * 768} Cout768 split256']), ('slot_sum_kernel', ['slots1 E768 Cout768 split256'])], 'q|k|v')
    assert len(out) == 6 and all(t.abs().max() > 0 for t in out)


@pytest.mark.parametrize('C,vpl', [(64, 1), (512, 2)])
def test_norm_backward_chain(C, vpl):
    from video_diffusion_nnx_amd import _lib as L, ops
    B, G, pix = 2, 8, 32
    y, dact, r = _randn(B, 1, 4, 8, C, seed=5), _randn(B, 1, 4, 8, C, seed=6), _randn(B, 1, 4, 8, C, seed=7)
    gamma, beta, ln_gamma = _randn(C, seed=8), _randn(C, seed=9), _randn(C, seed=10)
    yg = y.double().reshape(B, pix, G, C // G)
    stats = torch.zeros(B, L.GN_SLOTS, G, 2, dtype=torch.float64, device=DEV)
    stats[:, 0, :, 0], stats[:, 0, :, 1] = yg.sum((1, 3)), (yg * yg).sum((1, 3))
    stats = stats.reshape(-1)
    nwg = (ops._norm_bwd_scr(C, B, pix) - 64 * B) // (4 * B * C)          # workgroups per sample of the reduce pass, by the scratch it is given
    assert nwg == {64: 1, 512: 2}[C]
    for ln in (1, 0):
        kw = dict(r=r, ln_gamma=ln_gamma) if ln else dict(scale_shift=_randn(B, 2 * C, seed=11))
        rec, out = _hooked_and_plain(lambda: ops.norm_act_backward_ex(dact, y, stats, gamma, beta, G, deterministic=True, **kw))
        tail = f'C{C} batch{B} pix{pix} nwg{nwg} ln {ln} ss {1 - ln} dss {1 - ln} dgp 1'
        assert_launches(rec, [('norm_bwd_reduce_kernel', [f'<{vpl}> {tail}']), ('norm_bwd_finalize_kernel', [f'ct{max(8, C // G)} {tail}']),
                              ('norm_bwd_apply_kernel', [f'<{vpl}> {tail}'])], f'norm backward C {C} ln {ln}')


@pytest.mark.parametrize('dtype,operands,a,b,targs', [(F32, False, 'sla_bwd_a_kernel', 'sla_bwd_b_kernel', ''), (F32, True, 'sla_bwd_a16_kernel', 'sla_bwd_b16_kernel', '<io16 0> '),
                                                      (BF, True, 'sla_bwd_a16_kernel', 'sla_bwd_b16_kernel', '<io16 1> ')])
def test_sla_core_passes(dtype, operands, a, b, targs):
    from video_diffusion_nnx_amd import ops
    NF, N = 2, 16
    q, k, v, d_out = (_randn(NF * N, 256, seed=20 + i, dtype=dtype) for i in range(4))
    rec, _ = _hooked_and_plain(lambda: ops.sla_core_backward_io(q, k, v, d_out, NF, N, bf16_operands=operands))
    assert_launches(rec, [(a, [f'{targs}N{N} NF{NF} heads8']), (b, [f'{targs}N{N} NF{NF} heads8'])], f'SLA core {dtype} operands {operands}')
    assert rec[0][1] == rec[1][1]


def test_final_conv_backward_chain():
    from video_diffusion_nnx_amd import ops
    D = 16
    x, d_out, kernel = _ints(1, 2, 4, 4, D, seed=30), _ints(1, 2, 4, 4, 1, seed=31), _ints(1, D, 1, seed=32)      # (exact sums: the atomics below give the same bits on every run)
    scratch = torch.empty(1024, dtype=F32, device=DEV)
    rec, _ = _hooked_and_plain(lambda: ops.final_conv_backward(x, d_out, kernel, scratch=scratch))
    assert_launches(rec, [('final_conv_dx_kernel', [f'D{D} Cout1 npix32']), ('final_conv_dw_kernel', ['<x16 0>', f'D{D} Cout1 npix32 slots2 det 1']),
                          ('slot_sum_kernel', [f'slots2 E{D} Cout1 split0']), ('slot_sum_kernel', ['slots2 E1 Cout1 split0'])], 'head')
    rec, _ = _hooked_and_plain(lambda: ops.final_conv_backward(x, d_out, kernel))
    assert_launches(rec, [('final_conv_dx_kernel', []), ('final_conv_dw_kernel', ['det 0'])], 'head without scratch')


@pytest.mark.parametrize('nlayers,kb', [(2, 1), (8, 8)])
def test_scale_shift_backward_chain(nlayers, kb):
    from video_diffusion_nnx_amd import ops
    B, temb_dim, n = 2, 64, 32
    layers, off = [], 0
    for l in range(nlayers):
        layers.append(dict(w_off=off, b_off=off + temb_dim * n, g_off=off + temb_dim * n + n, be_off=off + temb_dim * n + 2 * n, out_off=l * n, n=n))
        off += temb_dim * n + 3 * n
    params, temb, lin = _randn(off, seed=40), _randn(B, temb_dim, seed=41), _randn(nlayers * n * B, seed=42)
    scratch = torch.empty(nlayers * B * temb_dim, dtype=F32, device=DEV)

    def run():
        grads, dss, dtemb = torch.zeros_like(params), _randn(nlayers * n * B, seed=43), torch.zeros(B, temb_dim, device=DEV)
        ops.resblock_scale_shift_backward(params, grads, temb, layers, lin, dss, dtemb, scratch=scratch)
        return grads, dss, dtemb

    rec, out = _hooked_and_plain(run)
    what = f'layers{nlayers} temb{temb_dim} B{B}'
    assert_launches(rec, [('resblock_ss_bwd_kernel', [what]), ('resblock_ss_bwd_w_kernel', [f'{what} kb{kb} det 1']),
                          ('slot_sum_kernel', [f'slots{nlayers} E{B * temb_dim} Cout{temb_dim} split0'])], f'scale/shift backward, {nlayers} layers')
    assert all(t.abs().max() > 0 for t in out)


@pytest.mark.parametrize('nslots,kernel', [(31, 'slot_sum_kernel'), (32, 'slot_sum16_kernel')])
def test_slot_sum_kernels(nslots, kernel):
    from video_diffusion_nnx_amd import ops
    E = 100
    part = _ints(nslots, E, seed=50)
    rec, out = _hooked_and_plain(lambda: ops.slot_sum(part, nslots, E, E, [torch.ones(E, device=DEV)]))
    assert_launches(rec, [(kernel, [f'slots{nslots} E{E} Cout0 split0'])], f'{nslots} slots')
    assert torch.equal(out[0], 1 + part.sum(0))
