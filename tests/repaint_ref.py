"""CPU restatement of RePaint resampling (test infrastructure), written independently of eo_diffusion_amd/diffusion:

  resample_schedule   the walk as a CLOSED FORM over blocks instead of the product's level-by-level simulation: jumps never nest (a jump
                      from point p lands on p + L, the jump point above, and landing triggers nothing), so the walk is the levels above
                      the top block once, then for every jump point p from the top down the block [p + L, ..., p + 1] U times, then
                      level 0;
  renoise_coeffs      (ca, cb) of the forward move in numpy fp32, correctly rounded sqrt (oracle.sampler_ref._sqrt explains why numpy);
  renoise             ca * x + cb * z in separately rounded torch fp32 operations;
  ddpm_resampled      the resampled DDPM / DDIM loops assembled from oracle.sampler_ref's step functions;
  ddim_resampled
  EVALS, MOVES        the walk and every Philox key of T = 8, resample = (2, 2), written out by hand.
"""
import numpy as np
import torch

from oracle import sampler_ref as SR


# T = 8, resample = (2, 2), written out by hand: the 14 evaluations as (timestep, Philox stream id of its mix / step noise), and after
# evaluation number k (from 1) the move (from level, to level, (step, stream id) of its noise)
EVALS = [(7, 1), (6, 1), (5, 1), (6, 3), (5, 3), (4, 1), (3, 1), (4, 3), (3, 3), (2, 1), (1, 1), (2, 3), (1, 3), (0, 1)]
MOVES = {3: (4, 6, (6, 2)), 7: (2, 4, (4, 2)), 11: (0, 2, (2, 2))}


def resample_schedule(num_levels, jump_length, jump_n_sample):
    n, L, U = int(num_levels), int(jump_length), int(jump_n_sample)
    points = list(range(0, n - L, L))
    if not points:
        return list(range(n - 1, -1, -1)), []
    visits = list(range(n - 1, points[-1] + L, -1))      # above the top block: visited once
    jumps = []
    for p in reversed(points):
        block = list(range(p + L, p, -1))
        for rep in range(U):
            visits += block
            if rep < U - 1:
                jumps.append((len(visits), p, p + L))
    return visits + [0], jumps


def walk_of(num_levels, resample):
    """(levels visited in order, the evaluation numbers (from 1) a jump follows); resample None: the single descent"""
    if resample is None:
        return list(range(num_levels - 1, -1, -1)), set()
    visits, jumps = resample_schedule(num_levels, *resample)
    return visits, {k for k, _, _ in jumps}


def renoise_coeffs(acp_from, acp_to):
    """fp32 (ca, cb): r = acp_to / acp_from, ca = sqrt(r), cb = sqrt(1 - r), each operation rounded once"""
    r = np.float32(acp_to) / np.float32(acp_from)
    return np.sqrt(r), np.sqrt(np.float32(1.0) - r)


def renoise(x, z, acp_from, acp_to):
    ca, cb = renoise_coeffs(acp_from, acp_to)
    assert ca.dtype == np.float32 and cb.dtype == np.float32 and x.dtype == torch.float32 and z.dtype == torch.float32
    p = x * float(ca)      # (a python float times an fp32 tensor is an fp32 multiply by the fp32 value ca is)
    q = z * float(cb)
    return p + q


def ddpm_resampled(tb, eps_fn, x_T, noises, jump_noises, timesteps, resample, clip=True, gt=None, mask=None):
    """oracle.sampler_ref.ddpm_sampling over the resampled walk: noises[k] belongs to evaluation k of the walk, jump_noises[j] to jump j"""
    visits, jumps = resample_schedule(timesteps, *resample)
    after = {k: (j, a, b) for j, (k, a, b) in enumerate(jumps)}
    acp = tb["alphas_cumprod"]
    x_t, n = x_T, x_T.shape[0]
    for k, i in enumerate(visits):
        t = torch.full((n,), i, dtype=torch.int64)
        if gt is not None:
            x_t = SR.repaint_mix(tb, x_t, gt, mask, t, noises[k])
        pred = eps_fn(x_t, t)
        x_t = (SR.ddpm_step_clip if clip else SR.ddpm_step_noclip)(tb, x_t, t, noises[k], pred)
        if k + 1 in after:
            j, a, b = after[k + 1]
            x_t = renoise(x_t, jump_noises[j], acp[a].item(), acp[b].item())
    return x_t


def ddim_resampled(tb, dd, steps, eps_fn, x_T, step_noises, jump_noises, resample, x0=None, mask=None, mix_noises=None):
    """oracle.sampler_ref.ddim_sampling over the resampled walk of the INDICES into `steps`; the move a -> b reads dd["a"] at both"""
    visits, jumps = resample_schedule(len(steps), *resample)
    after = {k: (j, a, b) for j, (k, a, b) in enumerate(jumps)}
    img, n = x_T, x_T.shape[0]
    pred_x0 = img
    for i, index in enumerate(visits):
        ts = torch.full((n,), int(steps[index]), dtype=torch.long)
        if mask is not None:
            img = SR.q_sample(tb, x0, ts, mix_noises[i]) * mask + (1.0 - mask) * img
        e_t = eps_fn(img, ts)
        img, pred_x0 = SR.ddim_step(img, e_t, dd["a"][index], dd["a_prev"][index], dd["sigma"][index], dd["sqrt_1m_a"][index], step_noises[i])
        if i + 1 in after:
            j, a, b = after[i + 1]
            img = renoise(img, jump_noises[j], float(dd["a"][a]), float(dd["a"][b]))
    return img, pred_x0
