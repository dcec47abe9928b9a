"""Parity of the ResnetBlock time-MLP backward on its own: resblock_ss_bwd_kernel (the LayerNorm backward per (layer, sample)) +
resblock_ss_bwd_w_kernel (the Linear's, one or eight rows per workgroup) + the fixed-order sum of the per-layer d(temb) slots, through
vdx_resblock_scale_shift_backward, which calls launch_resblock_ss_bwd exactly as model_bwd.hip's ss_bwd() does.

Cases, fp64 references and bounds come from tests/_ss_backward_cases.py (reference side alone: max(2e-6, 8 x CPU fp32) per group, every
figure printed -- run with -s).  Every case runs with the network's slot scratch (NaN-filled before each run; twice, bit-identical), with
float atomics (no scratch) and with a scratch reported one float too small (atomics again); a second call onto the first one's grads and
d(temb) must give exactly twice the first result; the table cut into stages in reverse order must give the reference of the whole table;
and nothing but the outputs may change: params, temb, lin, the sentinel gaps of grads and dss, the rows of layers outside a call, the
scratch beyond nlayers * B * temb_dim.  tests/test_host_parity_helpers.py shows on the CPU which kernel faults these bounds reject and
the whole-network per-tensor bound does not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bwd_parity_routes as BR
import _parity as P
import _ss_backward_cases as SC
from oracle import unet3d_ref as R

DEV = 'cuda:0'
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _dev(t, dtype=F32):
    return None if t is None else t.detach().to(dtype).to(DEV).contiguous()


@pytest.fixture(scope='module')
def slots():
    """The slot scratch the network hands launch_resblock_ss_bwd (12 Mi floats)."""
    from video_diffusion_nnx_amd import ops
    return torch.full((ops.WG_PART_FLOATS,), float('nan'), dtype=F32, device=DEV)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class _Run:
    """Device buffers of one case; call(which) runs the entry point over the layers `which` of the table."""

    def __init__(self, c):
        self.c = c
        self.params, self.temb, self.lin = _dev(c['params']), _dev(c['temb']), _dev(c['lin'])
        grads0 = torch.zeros(c['total'], dtype=F32)
        grads0[SC.gap_mask(c['layers'], c['temb_dim'], c['total'])] = SC.SENTINEL
        self.grads0 = grads0
        self.fresh()

    def fresh(self):
        self.grads, self.dss = _dev(self.grads0), _dev(self.c['dss'])
        self.dtemb = torch.zeros(self.c['B'], self.c['temb_dim'], dtype=F32, device=DEV)

    def call(self, which=None, scratch=None, short=False):
        from video_diffusion_nnx_amd import ops
        c = self.c
        layers = c['layers'] if which is None else [c['layers'][i] for i in which]
        need = len(layers) * c['B'] * c['temb_dim']
        if scratch is not None:
            scratch.fill_(float('nan'))          # every run: a slot read without having been written in THIS call shows
        label = 'short' if short else ('atomics' if scratch is None else 'slots')
        with BR.bound(BR.cid('ss', c['name'], len(layers), label), det=label == 'slots'):
            ops.resblock_scale_shift_backward(self.params, self.grads, self.temb, layers, self.lin, self.dss, self.dtemb, scratch=scratch,
                                              scratch_floats=need - 1 if short else None)
        torch.cuda.synchronize()
        if scratch is not None:
            used = 0 if short else need
            assert torch.isnan(scratch[used:]).all(), f'{c["name"]}: the scratch behind {used} floats was written'
            assert short or torch.isfinite(scratch[:need]).all(), f'{c["name"]}: a slot was left unwritten'

    def outputs(self):
        return self.grads.cpu(), self.dss.cpu(), self.dtemb.cpu()

    def inputs_untouched(self):
        c = self.c
        assert _bits(self.params.cpu(), c['params']) and _bits(self.temb.cpu(), c['temb']) and _bits(self.lin.cpu(), c['lin']), \
            f'{c["name"]}: params / temb / lin were written'


def _check(c, grads, dss, dtemb, what, scale=1.0):
    """Every output group against the fp64 reference (x scale) at its bound; the gaps keep the sentinel."""
    B, ref = c['B'], c['ref']
    gaps = SC.gap_mask(c['layers'], c['temb_dim'], c['total'])
    assert (grads[gaps] == SC.SENTINEL).all(), f'{what}: a gap of grads was written'
    assert (dss[~SC.row_mask(c['layers'], c['cols'], B, range(len(c['layers'])))] == SC.SENTINEL).all(), f'{what}: a gap of dss was written'
    worst = []                                   # (rel / bound, rel, bound, which) of every tensor's worst group
    for i, (got, (bound, sb)) in enumerate(zip(SC.unpack_rows(dss, c['layers'], B), c['b_dlin'])):
        _, lab, r = P.assert_exact_products(got, ref['dlin'][i], bound, c['sl'], sb, None, f'{what} d(lin) layer {i} n{c["widths"][i]}')
        worst.append((r / sb.get(lab, bound), r, sb.get(lab, bound), f'd(lin) layer {i} {lab}'))
    for i, got in enumerate(SC.unpack_params(grads, c['layers'], c['temb_dim'])):
        for k, t in zip(('dW', 'db', 'dg', 'dbe'), got):
            r, _, _ = P.assert_exact_products(t, scale * ref[k][i], c['b_par'][k][i], what=f'{what} {k} layer {i} n{c["widths"][i]}')
            worst.append((r / c['b_par'][k][i], r, c['b_par'][k][i], f'{k} layer {i}'))
    _, lab, r = P.assert_exact_products(dtemb, scale * ref['dtemb'], c['b_dtemb'][0], c['sl'], c['b_dtemb'][1], None, f'{what} d(temb)')
    bt = c['b_dtemb'][1].get(lab, c['b_dtemb'][0])
    worst.append((r / bt, r, bt, f'd(temb) {lab}'))
    w = max(worst)
    print(f'[ss bwd worst] {what}: {w[3]} rel {w[1]:.3e} (bound {w[2]:.3e})')


@pytest.mark.parametrize('name', list(SC.CASES))
def test_resblock_scale_shift_backward(name, slots):
    c = SC.case(name)
    nl = len(c['layers'])
    run = _Run(c)
    got = {}
    for label, kw in (('slots', dict(scratch=slots)), ('slots again', dict(scratch=slots)), ('atomics', dict()),
                      ('slots one float short', dict(scratch=slots, short=True))):
        run.fresh()
        run.call(**kw)
        got[label] = run.outputs()
        _check(c, *got[label], f'{name} {label}')
    assert all(_bits(a, b) for a, b in zip(got['slots'], got['slots again'])), f'{name}: two runs with slots are not bit-identical'
    # the parameter gradients and d(lin) do not depend on how d(temb) is summed
    for label in ('atomics', 'slots one float short'):
        assert _bits(got[label][0], got['slots'][0]) and _bits(got[label][1], got['slots'][1]), f'{name} {label}: grads / d(lin) differ from the slot form'

    # accumulation: a second call (fresh d(scale|shift): the first call overwrote it) onto the first call's grads and d(temb): x + x is exact
    run.fresh()
    run.call(scratch=slots)
    run.dss = _dev(c['dss'])
    run.call(scratch=slots)
    grads2, dss2, dtemb2 = run.outputs()
    g1, d1, t1 = got['slots']
    twice = torch.where(SC.gap_mask(c['layers'], c['temb_dim'], c['total']), g1, g1 + g1)
    assert torch.equal(grads2, twice), f'{name}: a second call onto the first one\'s grads is not exactly twice the first'
    assert torch.equal(dtemb2, t1 + t1), f'{name}: a second call onto the first one\'s d(temb) is not exactly twice the first'
    assert _bits(dss2, d1)
    _check(c, grads2, dss2, dtemb2, f'{name} accumulated twice', scale=2.0)

    # staging: the table in groups, last group first, each call over its own layers only
    passes = []
    for rep in range(2):
        run.fresh()
        done = []
        for which in SC.stages(nl):
            before = run.dss.cpu()
            run.call(which, scratch=slots)
            done += which
            outside = ~SC.row_mask(c['layers'], c['cols'], c['B'], which)
            assert _bits(run.dss.cpu()[outside], before[outside]), f'{name}: a call over layers {which} wrote dss rows of other layers'
            if len(done) < nl:
                rest = [i for i in range(nl) if i not in done]
                for i, t4 in enumerate(SC.unpack_params(run.grads.cpu(), c['layers'], c['temb_dim'])):
                    assert i not in rest or all((t == 0).all() for t in t4), f'{name}: a call over layers {which} wrote grads of layer {i}'
        passes.append(run.outputs())
        _check(c, *passes[-1], f'{name} staged {SC.stages(nl)} pass {rep}')
    assert all(_bits(a, b) for a, b in zip(*passes)), f'{name}: two staged passes with slots are not bit-identical'
    assert _bits(passes[0][0], got['slots'][0]) and _bits(passes[0][1], got['slots'][1]), f'{name}: staged grads / d(lin) differ from one call'
    run.inputs_untouched()


# ---- the chain norm backward -> time-MLP backward of the blocks -> time-MLP backward of the stem ----------------------------------------

def _small_bound(ref32, ref64):
    """The rule of the small backward kernels (tests/test_gpu_backward_forms.py): 4 x the fp32 CPU evaluation against fp64, the floor not
    below one fp32 ulp."""
    return 4.0 * max(P.rel(ref32, ref64), 2.0 ** -23)


def test_chain_norm_backward_to_time_mlp_backward(slots):
    """Two blocks (C = 64, B = 3, pixels (2, 8, 8)) sharing one temb: vdx_norm_act_backward_ex (dss) -> vdx_resblock_scale_shift_backward
    -> vdx_time_mlp_backward.  Each stage against the fp64 reference computed from the tensor that stage actually READ (the previous
    kernel's output), and dw1, db1, dw2, db2 at the end against fp64 autograd of the whole chain."""
    from video_diffusion_nnx_amd import ops
    g = torch.Generator().manual_seed(77)
    mk = lambda *s: torch.randn(*s, generator=g)
    C, B, shape, dim = 64, 3, (2, 8, 8), 16
    td = 4 * dim                                                           # temb_dim = 64
    t = torch.tensor([3, 437, 999])
    w1, b1, w2, b2 = mk(dim, td) / dim ** 0.5, 0.1 * mk(td), mk(td, td) / td ** 0.5, 0.1 * mk(td)
    blocks = []
    for _ in range(2):
        blocks.append(dict(y=P.bf16r(mk(B, *shape, C) * 1.5 + 0.3), gamma=1 + 0.2 * mk(C), beta=0.2 * mk(C), dact=mk(B, *shape, C),
                           W=mk(td, 2 * C) / td ** 0.5, b=0.1 * mk(2 * C), g=1 + 0.1 * mk(2 * C), be=0.1 * mk(2 * C)))
    layers, total, cols = SC.layout((2 * C, 2 * C), td)
    tensors = [(k['W'], k['b'], k['g'], k['be']) for k in blocks]

    def forward(dt, leaves=None):
        """-> (temb, [lin], [ss], [out]) in dt; leaves: dict to collect the differentiable parameters"""
        ps = [p.to(dt).requires_grad_(True) for p in (w1, b1, w2, b2)]
        temb = R.gelu_tanh(R.sinusoidal_pos_emb(t, dim, dt) @ ps[0] + ps[1]) @ ps[2] + ps[3]
        lins, sss, outs = [], [], []
        for k in blocks:
            lin = R.silu(temb) @ k['W'].to(dt) + k['b'].to(dt)
            ss = R.layer_norm(lin, k['g'].to(dt), k['be'].to(dt))
            h = R.group_norm(k['y'].to(dt), k['gamma'].to(dt), k['beta'].to(dt), 8) * (ss[:, None, None, None, :C] + 1) + ss[:, None, None, None, C:]
            lins.append(lin); sss.append(ss); outs.append(R.silu(h))
        return ps, temb, lins, sss, outs

    def whole(dt):
        ps, temb, lins, sss, outs = forward(dt)
        return torch.autograd.grad(sum((o * k['dact'].to(dt)).sum() for o, k in zip(outs, blocks)), ps)

    end64, end32 = whole(F64), whole(F32)
    with torch.no_grad():
        _, temb64, lins64, sss64, _ = forward(F64)
    temb_r, lin_r, ss_r = temb64.float(), [l.float() for l in lins64], [s.float() for s in sss64]       # what the forward left in memory

    # stage 1: d(scale|shift) of each block from the norm backward's finalize pass
    dss_got = []
    for i, k in enumerate(blocks):
        def dss_ref(dt):
            ss = ss_r[i].to(dt).requires_grad_(True)
            h = R.group_norm(k['y'].to(dt), k['gamma'].to(dt), k['beta'].to(dt), 8) * (ss[:, None, None, None, :C] + 1) + ss[:, None, None, None, C:]
            return torch.autograd.grad(R.silu(h), ss, k['dact'].to(dt))[0]
        with BR.bound(BR.cid('ss chain', 'norm')):
            res = ops.norm_act_backward_ex(_dev(k['dact']), _dev(k['y'], BF), P.gn_stats_slab(k['y']).reshape(-1).to(DEV), _dev(k['gamma']), _dev(k['beta']), 8,
                                           scale_shift=_dev(ss_r[i]), dy_bf16=True, deterministic=True)
        torch.cuda.synchronize()
        dss_got.append(res['dss'].cpu())
        # the bound test_norm_act_backward_bf16_tensors holds this output to (NORM_FP32)
        rr = P.rel(dss_got[-1], dss_ref(F64))
        print(f'[chain] block {i} dss from the norm backward: rel {rr:.3e} (bound 3.0e-05; CPU fp32 {P.rel(dss_ref(F32), dss_ref(F64)):.1e})')
        assert rr < 3e-5

    # stage 2: the new entry point on the dss the kernel above produced
    ref2, ref2_32 = SC.reference(temb_r, tensors, lin_r, dss_got, F64), SC.reference(temb_r, tensors, lin_r, dss_got, F32)
    params, grads = _dev(SC.pack_params(layers, tensors, total)), torch.zeros(total, dtype=F32, device=DEV)
    dss, dtemb = _dev(SC.pack_rows(layers, dss_got, cols, B)), torch.zeros(B, td, dtype=F32, device=DEV)
    slots.fill_(float('nan'))
    with BR.bound(BR.cid('ss chain', 'ss'), det=True):
        ops.resblock_scale_shift_backward(params, grads, _dev(temb_r), layers, _dev(SC.pack_rows(layers, lin_r, cols, B)), dss, dtemb, scratch=slots)
    torch.cuda.synchronize()
    sl = P.sample_slices((B,))
    for i, got in enumerate(SC.unpack_rows(dss.cpu(), layers, B)):
        bound, sb, _ = P.norm_bound(ref2_32['dlin'][i], ref2['dlin'][i], sl)
        P.assert_exact_products(got, ref2['dlin'][i], bound, sl, sb, None, f'chain block {i} d(lin)')
    for i, got in enumerate(SC.unpack_params(grads.cpu(), layers, td)):
        for key, tt in zip(('dW', 'db', 'dg', 'dbe'), got):
            P.assert_exact_products(tt, ref2[key][i], P.norm_bound(ref2_32[key][i], ref2[key][i])[0], what=f'chain block {i} {key}')
    dtemb_got = dtemb.cpu()
    bound, sb, _ = P.norm_bound(ref2_32['dtemb'], ref2['dtemb'], sl)
    P.assert_exact_products(dtemb_got, ref2['dtemb'], bound, sl, sb, None, 'chain d(temb)')

    # stage 3: the stem's time MLP on the d(temb) the kernels above accumulated
    def stem(dt, dtemb_in):
        ps = [p.to(dt).requires_grad_(True) for p in (w1, b1, w2, b2)]
        return torch.autograd.grad(R.gelu_tanh(R.sinusoidal_pos_emb(t, dim, dt) @ ps[0] + ps[1]) @ ps[2] + ps[3], ps, dtemb_in.to(dt))

    with BR.bound(BR.cid('ss chain', 'time_mlp')):
        got3 = ops.time_mlp_backward(t.to(DEV), _dev(w1), _dev(b1), _dev(w2), _dev(b2), dtemb)
    torch.cuda.synchronize()
    ref3, ref3_32 = stem(F64, dtemb_got), stem(F32, dtemb_got)
    for nm, a, r64, r32, e64, e32 in zip(('dw1', 'db1', 'dw2', 'db2'), got3, ref3, ref3_32, end64, end32):
        a = a.cpu().reshape(r64.shape)
        bd, rr = _small_bound(r32, r64), P.rel(a, r64)
        print(f'[chain] {nm} from the d(temb) it read: rel {rr:.3e} (bound {bd:.3e})')
        assert rr < bd, (nm, rr, bd)
        bd, rr = _small_bound(e32, e64), P.rel(a, e64)
        print(f'[chain] {nm} end to end against autograd of the whole chain: rel {rr:.3e} (bound {bd:.3e})')
        assert rr < bd, (nm, rr, bd)
