"""The eleven sampling-loop entry points of libvdx by argument name (include/vdx.h), shared by tests/test_gpu_sample_loops.py and
tests/test_host_sample_loops.py.  A plain module: nothing here is collected."""

# the positional signatures of include/vdx.h, by argument name
_HEAD = 'h params packed img eps t_dev step_dev'
_HEAD_DPM = 'h params packed img eps hist t_dev step_dev'
_TAIL = 'ws ws_bytes batch use_graph stream'
_ANC = 'tables timesteps nsteps cond seed clip'
_SEQ = 'ac seq seq_len nsteps cond clip'
_DYN_ANC = 'percentile thres'
_DYN_SEQ = 'tables timesteps percentile thres'
_MASK = 'known mask mtab'
_CFG = 'cond_scale rescale scratch'
SIGS = {
    'p_sample_loop': f'{_HEAD} {_ANC} {_TAIL}',
    'p_sample_loop_dyn': f'{_HEAD} {_ANC} {_DYN_ANC} {_TAIL}',
    'p_sample_loop_masked': f'{_HEAD} {_ANC} {_DYN_ANC} {_MASK} resample {_TAIL}',
    'p_sample_loop_guided': f'{_HEAD} {_ANC} {_DYN_ANC} {_CFG} {_TAIL}',
    'ddim_sample_loop': f'{_HEAD} {_SEQ} {_TAIL}',
    'ddim_sample_loop_dyn': f'{_HEAD} {_SEQ} {_DYN_SEQ} {_TAIL}',
    'ddim_sample_loop_masked': f'{_HEAD} {_SEQ} {_DYN_SEQ} {_MASK} seed {_TAIL}',
    'ddim_sample_loop_guided': f'{_HEAD} {_SEQ} {_DYN_SEQ} {_CFG} {_TAIL}',
    'dpm_sample_loop': f'{_HEAD_DPM} {_SEQ} order {_DYN_SEQ} {_TAIL}',
    'dpm_sample_loop_masked': f'{_HEAD_DPM} {_SEQ} order {_DYN_SEQ} {_MASK} seed {_TAIL}',
    'dpm_sample_loop_guided': f'{_HEAD_DPM} {_SEQ} order {_DYN_SEQ} {_CFG} {_TAIL}',
}
# the nine variants (one graph slot each): entry, step kernel, advance kernel
VARIANTS = {
    'p': ('p_sample_loop_dyn', 'p_sample_kernel', 'advance_kernel'),
    'p_masked': ('p_sample_loop_masked', 'p_sample_masked_kernel', 'resample_advance_kernel'),
    'p_guided': ('p_sample_loop_guided', 'p_sample_kernel', 'advance_kernel'),
    'ddim': ('ddim_sample_loop_dyn', 'ddim_step_kernel', 'ddim_advance_kernel'),
    'ddim_masked': ('ddim_sample_loop_masked', 'ddim_step_masked_kernel', 'ddim_advance_kernel'),
    'ddim_guided': ('ddim_sample_loop_guided', 'ddim_step_kernel', 'ddim_advance_kernel'),
    'dpm': ('dpm_sample_loop', 'dpm_step_kernel', 'ddim_advance_kernel'),
    'dpm_masked': ('dpm_sample_loop_masked', 'dpm_step_masked_kernel', 'ddim_advance_kernel'),
    'dpm_guided': ('dpm_sample_loop_guided', 'dpm_step_kernel', 'ddim_advance_kernel'),
}
ENTRY_VARIANT = {'p_sample_loop': 'p', 'ddim_sample_loop': 'ddim', **{e: v for v, (e, _, _) in VARIANTS.items()}}


def fn(entry):
    from video_diffusion_nnx_amd import _lib as L
    from video_diffusion_nnx_amd import gaussian_diffusion as G
    return getattr(G, 'vdx_' + entry, None) or getattr(L, 'vdx_' + entry)
