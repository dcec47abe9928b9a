"""CPU proofs for tests/test_gpu_step_kernels.py: the comparisons of that file reject an emulated kernel with the faults its shapes were
chosen for (a channel index taken from the first lane of a quad, a missed second sweep of a grid-stride loop, a quantile off by one
rank), and the conditions its dyn_thres cases rest on hold (no asserted value under the clamp at 1, frac == 0 in every exact case, the
quantile helper is torch.quantile).  The same check() and the same bounds as the GPU file, on outputs made up on the CPU."""
import numpy as np
import pytest
import torch

import _step_cases as S
from _step_cases import F32, F64, OLD, STRADDLE, WRAP


def _p_sample_case(sh):
    I = S.step_inputs(sh.name, 5, 2.0)
    t = S.t_vec(sh, S.T_P)
    ref64, _ = S.p_sample_ref(I['x'], I['eps'], I['z'], t, True, S.thres_vec(sh), F64)
    ref32, _ = S.p_sample_ref(I['x'], I['eps'], I['z'], t, True, S.thres_vec(sh), F32)
    bound, rel, floor = S.floor_bound(S.P_TOL_NOISE, ref32, ref64)
    return I, t, ref64, ref32, bound, rel, floor


def test_geometry_of_the_shapes():
    """The numbers the issue states for WRAP, from the launchers' grid caps."""
    assert S.per(WRAP) == 2100004 and S.per(WRAP) % 4 == 0 and WRAP.fhw % 2 == 1
    quads2 = S.per(WRAP) // 4 - S.EW_BLOCKS * S.THREADS
    assert quads2 == 713                                                       # workgroups 0, 1 whole and 201 threads of workgroup 2
    assert (quads2 // S.THREADS, quads2 % S.THREADS) == (2, 201)
    for n_one in (524288,):                                                    # one-element kernels: 2048 x 256 threads
        assert S.per(WRAP) // n_one == 4 and (WRAP.B * S.per(WRAP)) // n_one == 8
    assert S.N_ADAM - S.ADAM_SWEEP == 2803 and S.N_ADAM % 4 == 3                # a wrap, then a 3-element scalar tail
    assert S.N_ACC > S.SWEEP4 and S.N_RANDN > S.SWEEP4 and S.N_AFFINE > S.EW_BLOCKS * S.THREADS
    assert S.per(STRADDLE) == 140 and S.per(S.RAGGED) == 105 and S.per(S.RAGGED) % 4 == 1
    straddling = [q for q in range(S.per(STRADDLE) // 4) if (4 * q) // STRADDLE.fhw != (4 * q + 3) // STRADDLE.fhw]
    assert straddling == [8, 17, 26]
    m = S.mask('STRADDLE', 'lanes')[0].reshape(-1, 4)
    assert {tuple(r.tolist()) for r in m} == {tuple((p >> k) & 1 for k in range(4)) for p in range(16)}
    m = S.mask('STRADDLE', 'chan')
    assert all(int(m[b].reshape(4, -1).all(1).sum()) == 2 for b in range(3))


def test_first_lane_channel_is_rejected_at_straddle_and_passes_at_the_old_shape():
    for sh, rejected in ((STRADDLE, True), (OLD, False)):
        I, t, ref64, ref32, bound, rel, floor = _p_sample_case(sh)
        wrong_eps = S.eps_first_lane_channel(sh, I['eps'])                     # channel-first already
        faulty, _ = S.p_sample_ref(I['x'], wrong_eps.permute(0, 2, 3, 4, 1), I['z'], t, True, S.thres_vec(sh), F32)
        print(f'{sh.name}: floor {floor:.3e}, bound {rel:.3e} x max(1, |ref|max)')
        S.check(ref32, ref64, bound, f'{sh.name} honest fp32')
        if rejected:
            assert not torch.equal(wrong_eps, S.cf(I['eps']))
            with pytest.raises(AssertionError):
                S.check(faulty, ref64, bound, f'{sh.name} first-lane channel')
        else:
            assert torch.equal(wrong_eps, S.cf(I['eps']))                     # fhw % 4 == 0: every quad lies in one channel
            S.check(faulty, ref64, bound, f'{sh.name} first-lane channel')


def test_missed_second_sweep_is_rejected_at_wrap():
    sh = WRAP
    I, t, ref64, ref32, bound, rel, floor = _p_sample_case(sh)
    assert int(S.second_sweep(sh).sum()) == sh.B * 4 * 713
    S.check(ref32, ref64, bound, 'WRAP honest fp32')
    for how in ('nan', 'stale'):
        with pytest.raises(AssertionError):
            S.check(S.miss_second_sweep(sh, ref32, how), ref64, bound, f'WRAP second sweep {how}')
    # the rel-L2 bound of the optimizer and loss-gradient cases sees 2803 stale elements of 4 197 107 as well
    r64, r32 = S.adam_ref(F64), S.adam_ref(F32)
    for k in ('p', 'dp', 'm', 'v', 'ema'):
        stale = r32[k].clone()
        stale[S.ADAM_SWEEP:] = (S.adam_inputs()[k] if k != 'dp' else torch.zeros(S.N_ADAM))[S.ADAM_SWEEP:]     # the tail never updated
        bd = S.small_bound(r32[k], r64[k])
        assert S.rel_l2(r32[k], r64[k]) < bd <= S.rel_l2(stale, r64[k]), k


def test_quantile_helper_is_torch_quantile():
    g = torch.Generator().manual_seed(0)
    for n in (1, 2, 3, 960, 4097):
        v = torch.randn(n, generator=g, dtype=F64).abs()
        for q in S.DYN_QS + S.EXACT_QS:
            q32 = float(np.float32(q))
            assert abs(S.quantile_ref(v.numpy(), q) - torch.quantile(v, q32).item()) <= 1e-14 * max(1.0, v.max().item()), (n, q)


def test_dyn_thres_gaussian_cases_sit_above_the_clamp():
    for per_sample, C in S.DYN_GAUSS:
        G = S.dyn_gauss(per_sample, C)
        for q, ref in G['ref'].items():
            assert (ref >= S.DYN_MARGIN).all(), (per_sample, C, q, ref)


def test_dyn_thres_exact_cases_have_frac_zero_and_reject_a_shifted_rank():
    for per_sample in S.EXACT_PERS:
        assert per_sample % 4 == 1 and per_sample > 1024
        for q in S.EXACT_QS:
            E = S.dyn_exact(per_sample, q)
            assert E['frac'] == 0.0 and E['k'] == round(float(np.float32(q)) * (per_sample - 1)), (per_sample, q)
            assert (E['want'] > S.DYN_MARGIN).all(), (per_sample, q, E['want'])
            for s in E['sorted']:
                assert s.dtype == np.float32 and np.isfinite(s).all()
                nz = s[s != 0]
                assert (nz >= np.finfo(np.float32).tiny).all()               # no denormals
            by = dict(zip(S.EXACT_PATTERNS, range(len(S.EXACT_PATTERNS))))
            k, n = E['k'], per_sample
            # what each pattern is for
            assert E['sorted'][by['equal']][0] == E['sorted'][by['equal']][-1]
            first, last, inside = E['sorted'][by['first']], E['sorted'][by['last']], E['sorted'][by['inside']]
            assert first[k] != first[k - 1]
            assert (last[k] != last[k + 1]) if k + 1 < n else (last[0] == last[-1])
            assert inside[k] == inside[k - 1] and (k + 1 == n or inside[k] == inside[k + 1])
            u = E['sorted'][by['lowbyte']].view(np.uint32)
            assert len(np.unique(u)) >= 64 and len(np.unique(u >> 8)) <= 4     # the last radix pass has to tell them apart
            dec = E['sorted'][by['decades']].view(np.uint32)
            assert len(np.unique(dec >> 24)) >= 40                             # many top-byte buckets
            zs = E['sorted'][by['zeros']]
            assert 0 < int((zs == 0).sum()) < k
            # a quantile one rank too low / too high is not the asserted bits in at least one pattern each
            assert (E['below'] != E['want']).any(), (per_sample, q)
            if k + 1 < n:
                assert (E['above'] != E['want']).any(), (per_sample, q)
    x = S.dyn_exact(4097, 0.5)['x']
    assert bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())      # both zeros


def test_off_by_one_rank_passes_the_gaussian_case_when_per_sample_is_large():
    """Why the exact cases exist: at 2 100 004 elements neighbouring order statistics are closer than rtol 1e-6."""
    G = S.dyn_gauss(2100004, 4)
    passes = 0
    for q in S.DYN_QS:
        for b in range(S.DYN_B):
            off = S.quantile_ref(G['mag'][b], q, shift=1)
            passes += abs(off - G['ref'][q][b]) <= S.DYN_ATOL + S.DYN_RTOL * abs(G['ref'][q][b])
    print(f'off-by-one quantiles inside rtol 1e-6 at per_sample 2 100 004: {passes} of {len(S.DYN_QS) * S.DYN_B}')
    assert passes > 0
