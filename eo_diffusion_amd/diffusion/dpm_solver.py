"""DPMSolverSampler: DPM-Solver++ (2M) -- the second-order multistep solver of the data-prediction form of the probability-flow ODE
(Lu et al. 2022) -- on the fused HIP kernel eod_dpmpp_step.  No counterpart in the reference; DESIGN.md section 9.4.

Per evaluation: [optional RePaint mask mix: eod_q_sample + eod_repaint_mix] -> UNet launch program (plain or guided estimate) ->
ONE eod_dpmpp_step: x0 prediction from the noise estimate, optional clamp, the multistep combination with the previous prediction, the
state update.  It writes the new state and the prediction, which is the next evaluation's history.  The per-step scalars are computed
once per call on the host in float64 (diffusion/util.py make_dpm_timesteps / dpm_coefficients, from ONE host copy of the model's
alphas_cumprod buffer) and handed over by value: nothing synchronises per step.

The walk is DDIMSampler's (chain.walk over the INDICES of the levels, resample=(jump_length, jump_n_sample) with eod_renoise between
the levels' cumulative alpha products); what it shares with DDIM (_eps, _walk, _after_step) is inherited.  First order is used on the
first evaluation, on the evaluation right after a resampling jump (the history belongs to another noise level and is dropped), on the
last step (index 0: lower-order final) and everywhere with order=1; the step body decides from the index of the evaluation before it,
so chain.walk does not know about the history.  Draw policy: DDIMSampler's minus the eta noise -- x_T, the mix noise when a mask is
given, one draw per jump.
`observation=` (a diffusion/consistency.py Observation) on sample / sample_scene: the prediction of every evaluation is made consistent
with an observation of per-channel block means inside the step kernel (eod_dpmpp_step_obs: after the clamp, before the multistep
combination; the history the next evaluation reads is the projected prediction).  DESIGN.md section 9.5.
A SpectralObservation (eod_dpmpp_step_spec) or a list of 1 .. 4 observations (eod_pred_x0, one projection per link, eod_dpmpp_step_p0: the
history is the last link's result) goes the same way; DESIGN.md section 9.6.
A PsfObservation is a link like the others; alone it runs as a chain of one.
`threshold=` (a diffusion/threshold.py DynamicThreshold) on sample / sample_scene: every evaluation's prediction is clamped to its own
quantile and rescaled in place of the static clamp -- eod_pred_x0 (clip = 0), eod_dyn_threshold, the observation's links if any,
eod_dpmpp_step_p0; the history is the thresholded (and projected) prediction.  DESIGN.md section 9.12.
A model with `parameterization="x0" | "v"` runs every call on that route, with no links when it has neither observation nor threshold:
eod_param_pred (no noise estimate: the solver needs none) forms the prediction directly from the raw output, then eod_dpmpp_step_p0;
DESIGN.md section 9.16.
"""
import numpy as np
import torch

from .. import _lib
from ..engine import current_stream_ptr, f32c, require_gpu
from . import consistency, threshold as thresholding
from .ddim import DDIMSampler
from .util import dpm_coefficients, dpm_lambda, make_dpm_timesteps, resample_plan


class DPMSolverSampler(DDIMSampler):
    # ------------------------------------------------------------------ host side: levels and per-step scalars
    def make_dpm_schedule(self, S, discretize="logsnr", t_start=None, order=2):
        """levels (ascending; self.num_evaluations of them) and the fp32 scalars of every step, from one host copy of the model's buffer"""
        if order not in (1, 2) or isinstance(order, bool):
            raise _lib.EodError(f"DPMSolverSampler: order is 1 or 2, got {order!r}")
        acp = self.model.alphas_cumprod.detach().cpu().numpy().astype(np.float32, copy=False)
        assert acp.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        levels = make_dpm_timesteps(discretize, S, acp, t_start)
        a = acp[levels]
        a_prev = np.concatenate([acp[:1], a[:-1]])
        h = dpm_lambda(a_prev) - dpm_lambda(a)
        n = len(levels)
        self.order = order
        self.dpm_timesteps = self.ddim_timesteps = levels
        self.num_evaluations = n
        self.ddim_alphas = a                     # (what _walk's eod_renoise moves between)
        self.dpm_alphas_prev = a_prev
        self.dpm_sqrt_one_minus_alphas = np.sqrt(np.float32(1.0) - a)   # fp32, as DDIMSampler.make_schedule has it
        self.dpm_first = [dpm_coefficients(a[i], a_prev[i]) for i in range(n)]
        self.dpm_second = [dpm_coefficients(a[i], a_prev[i], h[i + 1], 2) if order == 2 and 0 < i < n - 1 else None for i in range(n)]
        return levels

    def _plan(self, what, S, order, discretize, t_start, resample, mix_noises, jump_noises, mask, x0):
        """everything a call refuses, before any launch; returns (visits, jump_after)"""
        if (mask is None) != (x0 is None):
            raise _lib.EodError(f"{what}: mask and x0 go together (RePaint mix of the known region)")
        self.make_dpm_schedule(S, discretize, t_start, order)
        n = self.num_evaluations
        if resample is None and mix_noises is not None and len(mix_noises) != n:
            raise _lib.EodError(f"{what}: the call evaluates the UNet {n} times, `mix_noises` has {len(mix_noises)} entries")
        return resample_plan(what, resample, n, (("mix_noises", mix_noises),), jump_noises)

    # ------------------------------------------------------------------ the step
    def _dpm_update(self, x, e_t, hist, index, clip, obs=None):
        """(x_next, pred_x0) of the evaluation at step `index`; hist = (index, pred_x0) of the evaluation before it, or None; obs =
        (BoundObservation, number of the evaluation): eod_dpmpp_step_obs in place of eod_dpmpp_step"""
        second = self.dpm_second[index] if hist is not None and hist[0] == index + 1 else None
        c_x, c_d, w_cur, w_prev = self.dpm_first[index] if second is None else second
        x, e_t = f32c(x), f32c(e_t)
        d_prev = None if second is None else hist[1]
        if obs is None and self._parameterization() != "eps":   # an "x0" / "v" output: a chain with no links
            obs = (consistency.BoundChain([], parameterization=self._parameterization()), 0)
        if obs is not None:
            return obs[0].dpmpp_step(obs[1], x, e_t, d_prev, self.ddim_alphas[index], self.dpm_sqrt_one_minus_alphas[index], c_x, c_d, w_cur,
                                     w_prev, clip)
        x_next, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().eod_dpmpp_step(x.data_ptr(), e_t.data_ptr(), _lib.ptr(d_prev), float(self.ddim_alphas[index]),
                                             float(self.dpm_sqrt_one_minus_alphas[index]), float(c_x), float(c_d), float(w_cur),
                                             float(w_prev), int(bool(clip)), x_next.data_ptr(), pred_x0.data_ptr(), x.numel(),
                                             current_stream_ptr(x.device)), "eod_dpmpp_step")
        return x_next, pred_x0

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, *, order=2, discretize="logsnr", t_start=None, clip_denoised=False,
               mask=None, x0=None, x_T=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None, mix_noises=None,
               resample=None, jump_noises=None, callback=None, img_callback=None, log_every_t=100, progress=True, observation=None,
               threshold=None):
        """`S` steps (self.num_evaluations <= S UNet evaluations: duplicate levels of the logsnr grid are removed) from x_T to an image
        batch [batch_size, *shape].  Returns (samples, {"x_inter", "pred_x0"}) like DDIMSampler.sample.  mask / x0: the RePaint mix at
        every evaluation (mix_noises[i]: its q_sample noise, indexed by the evaluation's position in the walk).  resample /
        jump_noises: RePaint resampling over the indices of the levels, as in DDIMSampler.ddim_sampling.  observation: an Observation or a
        SpectralObservation for a state [batch_size, *shape], or a list of 1 .. 4 of them applied in order; a per-evaluation `weight` is
        indexed like mix_noises.  threshold: a DynamicThreshold (diffusion/threshold.py): every evaluation's prediction is formed without
        the static clamp, thresholded per batch member (or per band), then projected by the observation's links, if any; it REPLACES the
        clamp, so clip_denoised makes no difference to a call that has one.  pred_x0 in the intermediates and the history is the final
        prediction.  None: today's launches and bits."""
        what = "DPMSolverSampler.sample"
        visits, jump_after = self._plan(what, S, order, discretize, t_start, resample, mix_noises, jump_noises, mask, x0)
        device = self.model.betas.device
        C, H, W = shape
        b = batch_size
        obs = thresholding.bind(threshold, observation, what, (b, C, H, W), len(visits), device, self._parameterization())
        if conditioning is not None and conditioning.shape[0] != b:
            print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {b}")
        img = torch.randn((b, C, H, W), device=device) if x_T is None else f32c(x_T.to(device))
        require_gpu(img, what)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        if mask is not None:
            mask = self.model._broadcast_mask(mask, img)
            x0 = f32c(torch.as_tensor(x0).to(device))
        levels, total_steps = self.dpm_timesteps, self.num_evaluations
        hist = [None]

        def step(img, i, index, visit):
            ts = torch.full((b,), int(levels[index]), device=device, dtype=torch.long)
            if mask is not None:
                nz = mix_noises[i].to(device) if mix_noises is not None else torch.randn_like(x0)
                img = self.model._repaint_mix(img, x0, mask, ts, nz)
            e_t = self._eps(img, ts, conditioning, unconditional_guidance_scale, unconditional_conditioning)
            img, pred_x0 = self._dpm_update(img, e_t, hist[0], index, clip_denoised, None if obs is None else (obs, i))
            hist[0] = (index, pred_x0)
            return self._after_step(i, index, img, pred_x0, intermediates, callback, img_callback, log_every_t, total_steps)

        img = self._walk(img, visits, jump_after, step, jump_noises, lambda name, z: z.to(device), "DPM-Solver++ Sampler" if progress else None)
        return img, intermediates

    @torch.no_grad()
    def sample_scene(self, S, scene_size, *, overlap=0, tile_batch=16, conditioning=None, mask=None, x0=None, order=2, discretize="logsnr",
                     t_start=None, clip_denoised=False, x_T=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
                     mix_noises=None, callback=None, img_callback=None, log_every_t=100, progress=True, resample=None, jump_noises=None,
                     skip_known=False, n_scenes=1, observation=None, threshold=None):
        """The solver over a scene (or a stack of n_scenes) larger than the UNet's image size: DDIMSampler.sample_scene's arguments with
        the solver's keywords in place of `eta` / `step_noises`.  One scene-level state, one scene-level history tensor and ONE
        eod_dpmpp_step on [B, C, H, W] per evaluation; tiles, blending, guidance per chunk, conditioning, skip_known (keep_known at the
        end) and n_scenes as there.  With overlap = 0 and injected draws the result equals sample() on the tiles, bit for bit; with
        skip_known it equals the skip_known=False scene at every estimated pixel and is `x0` elsewhere (at a pixel that is not
        estimated the zero estimate keeps state and history finite; at an estimated pixel pred_x0 depends on that pixel's x and e only).
        observation: as in DDIMSampler.sample_scene (scene-sized, blocks anchored at the scene's origin, refused with skip_known).
        threshold: as in DDIMSampler.sample_scene (the quantile of the whole scene's prediction, per member of a stack; it replaces the
        clamp, so clip_denoised makes no difference; refused with skip_known)."""
        from ..tiling import keep_known
        what = "DPMSolverSampler.sample_scene"
        m = self.model
        walk = lambda: self._plan(what, S, order, discretize, t_start, resample, mix_noises, jump_noises, mask, x0)
        sc = self._scene_setup(what, scene_size, overlap, tile_batch, n_scenes, walk, mask, x0, skip_known, conditioning,
                               unconditional_conditioning, unconditional_guidance_scale, x_T, observation, threshold)
        if sc.known is not None:
            return sc.known, {"x_inter": [sc.known], "pred_x0": [sc.known]}
        img, x0, mask, B, device = sc.img, sc.x0, sc.mask, sc.B, sc.device
        levels, total_steps = self.dpm_timesteps, self.num_evaluations
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        hist = [None]

        def step(img, i, index, visit):
            t = int(levels[index])
            if mask is not None:
                nz = sc.as_scene("mix_noises[i]", mix_noises[i]) if mix_noises is not None else torch.randn_like(x0)
                img = m._repaint_mix(img, x0, mask, torch.full((B,), t, device=device, dtype=torch.long), nz)
            e_t = self._scene_eps(sc, img, t, unconditional_guidance_scale)
            img, pred_x0 = self._dpm_update(img, e_t, hist[0], index, clip_denoised, None if sc.obs is None else (sc.obs, i))
            hist[0] = (index, pred_x0)
            return self._after_step(i, index, img, pred_x0, intermediates, callback, img_callback, log_every_t, total_steps)

        img = self._walk(img, sc.visits, sc.jump_after, step, jump_noises, sc.as_scene, "DPM-Solver++ Sampler (scene)" if progress else None)
        return (img if sc.tiles is sc.full else keep_known(img, x0, sc.tiles)), intermediates

    # ------------------------------------------------------------------ DDIM's own entry points do not apply to this sampler
    def ddim_sampling(self, *args, **kwargs):
        raise NotImplementedError("DPMSolverSampler: use sample() / sample_scene(); ddim_sampling belongs to DDIMSampler")

    def p_sample_ddim(self, *args, **kwargs):
        raise NotImplementedError("DPMSolverSampler: use sample() / sample_scene(); p_sample_ddim belongs to DDIMSampler")
