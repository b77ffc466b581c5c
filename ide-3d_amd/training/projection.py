"""Latent projection with trainable noise maps.

The reference ships its projectors under inversion/training/projectors/ (w_projector_ide3d.py and four variants that differ in the shape
of the optimised latent).  Each of them optimises one w next to every `noise_const` buffer of `G.synthesis`, adds a noise regulariser to
the loss and re-normalises the maps after every optimiser step.  This module holds the three pieces of that step which are not the
generator itself:

  noise_regularization(maps)   the regulariser (w_projector_ide3d.py:114-122) as one autograd Function over ide3d_noise_reg /
                               ide3d_noise_reg_backward (csrc/noise_reg.hip): 3 + 1 launches for all maps instead of ~10 per pyramid level;
  normalize_noise_(maps)       the re-normalisation (:139-142) as ide3d_noise_normalize: 3 launches for all maps;
  project(G, target, c, ...)   the schedule of w_projector_ide3d.py:50-145 around them.

Both ops fall back to their torch definition (written out below from the formula) for anything the kernels do not take: CPU tensors, maps
that are not square powers of two in 4..512, non-contiguous views, other dtypes, or `fused_noise_ops = False`.  The generator's part of the
step - a frozen layer with a trainable noise map on the HIP gradient path - is `networks.hip_noise_grad`.
"""

import copy

import numpy as np
import torch
import torch.nn.functional as F

# True: fp32 CUDA maps that are square powers of two in 4..512 and contiguous go through csrc/noise_reg.hip.  False: always the torch definition.
fused_noise_ops = True


def _fused(maps):
    if not (fused_noise_ops and len(maps) > 0):
        return False
    from torch_utils import hip_plugin
    return all(hip_plugin.NoisePlugin.supported(t) for t in maps) and all(t.device == maps[0].device for t in maps)


def _levels(n):
    """The pyramid of one [H, W] map: the map, then 2x2 average pools of it while the height is above 8."""
    a = n[None, None]
    yield a[0, 0]
    while a.shape[2] > 8:
        a = F.avg_pool2d(a, kernel_size=2)
        yield a[0, 0]


def _noise_regularization_torch(maps):
    """sum over maps and pyramid levels of mean(n * roll(n, 1, x))^2 + mean(n * roll(n, 1, y))^2, rolls wrapping around."""
    total = None
    for n in maps:
        for a in _levels(n):
            for dim in (1, 0):
                term = (a * torch.roll(a, shifts=1, dims=dim)).mean().square()
                total = term if total is None else total + term
    return total


class _NoiseReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *maps):
        from torch_utils import hip_plugin
        loss, means, ws = hip_plugin.NoisePlugin.noise_reg(list(maps))
        ctx.save_for_backward(*maps, means, ws)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from torch_utils import hip_plugin
        *maps, means, ws = ctx.saved_tensors
        grads = hip_plugin.NoisePlugin.noise_reg_backward(maps, ws, means, dloss.to(torch.float32))
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


def noise_regularization(maps):
    """The projectors' noise regulariser (reference w_projector_ide3d.py:114-122) of a list of [H, W] noise maps -> scalar tensor,
    differentiable with respect to every map.  An empty list gives zero."""
    maps = list(maps)
    if len(maps) == 0:
        return torch.zeros([])
    if _fused(maps):
        return _NoiseReg.apply(*maps)
    return _noise_regularization_torch(maps)


def normalize_noise_(maps):
    """In place, for every map: n -= mean(n); n *= rsqrt(mean(n^2)) (reference w_projector_ide3d.py:139-142, its no_grad included: the maps
    may be leaves that require grad).  Returns the list."""
    maps = list(maps)
    with torch.no_grad():
        if _fused(maps):
            from torch_utils import hip_plugin
            hip_plugin.NoisePlugin.noise_normalize(maps)
        else:
            for n in maps:
                n -= n.mean()
                n *= n.square().mean().rsqrt()
    return maps


def noise_maps(G):
    """Every const noise map of `G.synthesis`, in module order (reference w_projector_ide3d.py:64)."""
    return [buf for name, buf in G.synthesis.named_buffers() if 'noise_const' in name]


def l2_distance(target):
    """The default `distance` of `project`: the squared L2 distance to `target` [1, C, H, W] (0..255), both images area-down-sampled to
    256 x 256 when larger (the resolution the reference feeds its feature network, w_projector_ide3d.py:73-74, 106-107)."""
    def small(img):
        return F.interpolate(img, size=(256, 256), mode='area') if img.shape[2] > 256 else img
    target_small = small(target)
    return lambda images: (small(images) - target_small).square().sum()


class Projector:
    """The state of one projection and its step: what `project` loops over (scripts/bench_projector.py times the same step).  Arguments as
    for `project`."""

    def __init__(self, G, target, c, *, num_steps=1000, w_avg_samples=10000, initial_learning_rate=0.01, initial_noise_factor=0.05,
                 lr_rampdown_length=0.25, lr_rampup_length=0.05, noise_ramp_length=0.75, regularize_noise_weight=1e5,
                 distance=None, initial_w=None, device=None, camera_lr=None, camera_project=None):
        assert tuple(target.shape) == (G.img_channels, G.img_resolution, G.img_resolution)
        if device is None:
            device = next(G.parameters()).device
        device = torch.device(device)
        self.G = G = copy.deepcopy(G).eval().requires_grad_(False).to(device).float()
        self.num_ws = G.mapping.num_ws
        self.c = c = c.to(device=device, dtype=torch.float32)
        self.num_steps, self.initial_learning_rate, self.initial_noise_factor = num_steps, initial_learning_rate, initial_noise_factor
        self.lr_rampdown_length, self.lr_rampup_length, self.noise_ramp_length = lr_rampdown_length, lr_rampup_length, noise_ramp_length
        self.regularize_noise_weight = regularize_noise_weight

        with torch.no_grad():
            z = torch.from_numpy(np.random.RandomState(123).randn(w_avg_samples, G.z_dim)).to(device=device, dtype=torch.float32)
            w_samples = G.mapping(z, c.repeat(w_avg_samples, 1))[:, :1, :]                       # [N, 1, w_dim]
            w_avg = w_samples.mean(dim=0, keepdim=True)                                            # [1, 1, w_dim]
            self.w_std = float(((w_samples - w_avg).square().sum() / w_avg_samples).sqrt())
        start = w_avg if initial_w is None else torch.as_tensor(initial_w, dtype=torch.float32, device=device)
        assert start.ndim == 3 and start.shape[0] == 1 and start.shape[1] in (1, self.num_ws) and start.shape[2] == G.w_dim
        self.w_opt = start.detach().clone().requires_grad_(True)

        self.maps = noise_maps(G)
        with torch.no_grad():
            for n in self.maps:
                n.copy_(torch.randn_like(n))
        for n in self.maps:
            n.requires_grad_(True)
        self.optimizer = torch.optim.Adam([self.w_opt] + self.maps, betas=(0.9, 0.999), lr=initial_learning_rate)
        self.camera_lr, self.camera_project, self.cam_opt = camera_lr, camera_project, None
        if camera_lr is not None:
            # the 16 extrinsic entries of c train in a parameter group of their own; the 9 intrinsics stay what the caller passed
            self.cam_opt = c[:, :16].detach().clone().requires_grad_(True)
            self.intrinsics = c[:, 16:].detach()
            self.optimizer.add_param_group(dict(params=[self.cam_opt], lr=camera_lr))
        self.distance = distance if distance is not None else l2_distance(target[None].to(device=device, dtype=torch.float32))

    def step(self, step):
        """Step number `step` of `num_steps` -> the loss (a device scalar; nothing here waits for the device)."""
        t = step / self.num_steps
        w_noise_scale = self.w_std * self.initial_noise_factor * max(0.0, 1.0 - t / self.noise_ramp_length) ** 2
        lr_ramp = min(1.0, (1.0 - t) / self.lr_rampdown_length)
        lr_ramp = 0.5 - 0.5 * np.cos(lr_ramp * np.pi)
        lr_ramp = lr_ramp * min(1.0, t / self.lr_rampup_length)
        if self.cam_opt is not None:
            return self._step_with_camera(w_noise_scale, lr_ramp)
        for group in self.optimizer.param_groups:
            group['lr'] = self.initial_learning_rate * lr_ramp

        ws = self.w_opt + torch.randn_like(self.w_opt) * w_noise_scale
        if ws.shape[1] == 1:
            ws = ws.repeat([1, self.num_ws, 1])
        images = self.G.synthesis(ws, c=self.c, noise_mode='const', force_fp32=True)
        images = (images + 1) * (255 / 2)
        loss = self.distance(images) + self.regularize_noise_weight * noise_regularization(self.maps)

        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        normalize_noise_(self.maps)
        return loss.detach()

    def camera(self):
        """The camera label [1, 25] as it stands: the refined extrinsics beside the caller's intrinsics (`c` itself without `camera_lr`)."""
        return self.c if self.cam_opt is None else torch.cat([self.cam_opt.detach(), self.intrinsics], 1)

    def _step_with_camera(self, w_noise_scale, lr_ramp):
        """`step` with the pose as a second parameter group (learning rate `camera_lr` under the same ramp).  The renderer's camera switch
        (triplane.fused_render_camera_grad) is on for the pass and restored after it."""
        from training import triplane
        self.optimizer.param_groups[0]['lr'] = self.initial_learning_rate * lr_ramp
        self.optimizer.param_groups[1]['lr'] = self.camera_lr * lr_ramp
        ws = self.w_opt + torch.randn_like(self.w_opt) * w_noise_scale
        if ws.shape[1] == 1:
            ws = ws.repeat([1, self.num_ws, 1])
        old, triplane.fused_render_camera_grad = triplane.fused_render_camera_grad, True
        try:
            images = self.G.synthesis(ws, c=torch.cat([self.cam_opt, self.intrinsics], 1), noise_mode='const', force_fp32=True)
            images = (images + 1) * (255 / 2)
            loss = self.distance(images) + self.regularize_noise_weight * noise_regularization(self.maps)
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
        finally:
            triplane.fused_render_camera_grad = old
        self.optimizer.step()
        normalize_noise_(self.maps)
        if self.camera_project is not None:
            with torch.no_grad():
                self.cam_opt.copy_(self.camera_project(self.cam_opt.detach().clone()))
        return loss.detach()

    def pivot(self):
        w = self.w_opt.detach()
        return w.repeat([1, self.num_ws, 1]) if w.shape[1] == 1 else w.clone()


def project(G, target, c, *, num_steps=1000, w_avg_samples=10000, initial_learning_rate=0.01, initial_noise_factor=0.05,
            lr_rampdown_length=0.25, lr_rampup_length=0.05, noise_ramp_length=0.75, regularize_noise_weight=1e5,
            distance=None, initial_w=None, device=None, return_info=False, camera_lr=None, camera_project=None):
    """Project `target` ([C, H, W], 0..255, the generator's output resolution) seen from camera label `c` ([1, 25]) into W with trainable
    noise maps: the schedule of the reference's w_projector_ide3d.py:50-145.  Returns the pivot [1, num_ws, w_dim].

    Works on a frozen float32 deep copy of G on `device` (default: where G's parameters are); the caller's G is left untouched.
      * w_avg, w_std from `w_avg_samples` latents of RandomState(123) mapped under `c` (:54-59); start at `initial_w` or w_avg (:61).
      * Every `noise_const` of the copy is re-drawn and made trainable (:83-85); Adam(betas 0.9, 0.999) over [w_opt] + maps (:79).
      * Per step: learning rate = initial_learning_rate * cosine ramp-down over the last `lr_rampdown_length` * linear ramp-up over the
        first `lr_rampup_length` (:92-97); w noise of scale w_std * initial_noise_factor * max(0, 1 - t / noise_ramp_length)^2 (:91, 100);
        images = G.synthesis(ws, c, noise_mode='const', force_fp32=True) (:102), mapped to 0..255 (:105);
        loss = distance(images) + regularize_noise_weight * noise_regularization(maps) (:111-123); step; normalize_noise_(maps) (:139-142).
    Defaults as in the reference's signature: num_steps 1000 (:29), w_avg_samples 10000 (:30), initial_learning_rate 0.01 (:31),
    initial_noise_factor 0.05 (:32), lr_rampdown_length 0.25 (:33), lr_rampup_length 0.05 (:34), noise_ramp_length 0.75 (:35),
    regularize_noise_weight 1e5 (:36), initial_w None (:40).

    distance: callable(images [1, C, H, W] in 0..255) -> scalar.  The reference measures LPIPS with VGG16 features of the 256 x 256
    area-down-sampled images (:66-75, 104-111); those weights are a download this project does not make, so the default is `l2_distance`
    (squared L2 of the same down-sampled images) and a caller with the feature network passes its LPIPS closure, e.g.
    `lambda img: (target_features - vgg16(F.interpolate(img, (256, 256), mode='area'), resize_images=False, return_lpips=True)).square().sum()`.
    With this package's feature network: `distance=training.lpips.lpips_distance(target[None], training.lpips.LPIPS('vgg'))` (weights loaded by the caller).

    The other projectors of the reference differ only in the latent: an `initial_w` of shape [1, num_ws, w_dim] is optimised per layer
    (w_plus_projector*.py); for the join-view variant pass a `distance` that renders and compares the second view itself.

    camera_lr: None (default) = `c` is fixed, the reference's schedule statement for statement.  A number = the 16 extrinsic entries of `c`
    (the flattened cam2world) are refined beside w: a second Adam parameter group with this learning rate under the same ramp; the 9
    intrinsics stay fixed.  On the GPU the renderer's gradient for the pose is ide3d_render_rays_backward_camera
    (`triplane.fused_render_camera_grad`, set for the duration of each pass and restored).  All 16 entries move freely: the rotation block
    is NOT re-orthonormalised and the last row is not pinned (its gradient is zero, so it stays).  `camera_project`: callable([1, 16]) ->
    [1, 16] applied under no_grad after every step (default: identity), e.g. a projection of the 3 x 3 block onto the nearest rotation.

    return_info: also return a dict with `losses` (one float per step), `noise_maps` (the copy's maps after the last step) and `w_std`;
    with `camera_lr`, also `c` (the refined camera label [1, 25])."""
    p = Projector(G, target, c, num_steps=num_steps, w_avg_samples=w_avg_samples, initial_learning_rate=initial_learning_rate,
                  initial_noise_factor=initial_noise_factor, lr_rampdown_length=lr_rampdown_length, lr_rampup_length=lr_rampup_length,
                  noise_ramp_length=noise_ramp_length, regularize_noise_weight=regularize_noise_weight, distance=distance,
                  initial_w=initial_w, device=device, camera_lr=camera_lr, camera_project=camera_project)
    losses = [p.step(step) for step in range(num_steps)]
    if return_info:
        info = dict(losses=[float(v) for v in losses], noise_maps=[n.detach() for n in p.maps], w_std=p.w_std)
        if camera_lr is not None:
            info['c'] = p.camera()
        return p.pivot(), info
    return p.pivot()
