"""The CLIP image-text loss with a HIP forward and image gradient.

Reference: the loss of the text-guided editing the reference vendors (inversion/models/StyleCLIP/criteria/clip_loss.py:6-17, used at
mapper/training/coach.py:206-209 and optimization/run_optimization.py:49-62) and of the README's "3D-aware CLIP-guided domain adaptation":

    image = AvgPool2d(stylegan_size // 32)(Upsample(scale_factor=7)(image))        # any S = 32 m -> 224 x 224
    loss  = 1 - logits_per_image / 100                                              # = 1 - cos(E_img(image), E_txt(text)), [n, T]

back-propagated through a frozen CLIP ViT-B/32 image encoder into the rendered image.  `VisionTransformer` here is written from the
definition of OpenAI CLIP's `visual` module with that module's parameter names and shapes, so the `visual.*` entries of a CLIP state
dict load unchanged (`load_clip_state_dict`, fp16 values included).  `CLIPLoss` has the reference's `forward(image, text)` on text
EMBEDDINGS and, for a training step, `distance_to` (its mean), `directional` (the StyleGAN-NADA loss against a frozen generator's
embeddings) and `features`; `clip_distance(...)` is the closure `training.projection.project(distance=...)` takes.

THE TEXT ENCODER AND ITS TOKENIZER STAY THE USER'S: their vocabulary is a download, and nothing here downloads.  Compute
`text_features = model.encode_text(clip.tokenize(prompts))` with any CLIP implementation whose image tower these weights come from and
pass the [T, D] result.  WITHOUT LOADED WEIGHTS THE NET IS RANDOMLY INITIALISED and the loss measures nothing; pass `weights=` (a path or a
state dict) or call `visual.load_clip_state_dict`.  StyleCLIP feeds images in [-1, 1] WITHOUT CLIP's own normalisation; that stays the
default (`mean = std = None`).  The bicubic 224 resize of the reference's `CLIPEncoder` (inversion/networks.py:1810-1816) is not reproduced.

`fused` (module switch, shipped False: see DESIGN.md section 5.37; set `clip_loss.fused = True`): float32 CUDA images [n, 3, S, S] with S a multiple of 32 and a `VisionTransformer` in eval mode whose parameters
are all frozen, with 224 % patch_size == 0, T = (224 / p)^2 + 1 <= 64 tokens, a head dimension that is a multiple of 4 and <= 64, width
and output_dim multiples of 4, run on the HIP path: one autograd Function whose forward launches ide3d_clip_prep, the dense products as
shared-weight 1x1 ide3d_modconv2d launches over channel-major token maps [n, C, T] (patch embedding, in_proj, out_proj, c_fc, c_proj),
ide3d_vit_embed, ide3d_layernorm, ide3d_vit_attention, ide3d_quickgelu, ide3d_residual_join, ide3d_linear on proj^T and ide3d_clip_head;
the backward launches the same products on the transposed weights and the adjoints of the other passes, and returns the image gradient
only.  Everything else - CPU tensors, other dtypes, trainable parameters, more than 64 tokens (ViT-B/16), text embeddings that require a
gradient, `fused = False` - is the plain PyTorch definition.  `CLIPLoss.last_path` is 'hip' or 'torch' after every call.
`arith` (module switch): the per-call arithmetic of the dense products on the HIP path (0 = the process default, see
`hip_plugin.conv_arithmetic`).
"""

import math
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from training import networks

# True: what the HIP path takes (see above) runs on it.  False: always the PyTorch definition.  Shipped False: the path's speed against the
# ATen path has not been measured yet; it is there for checking, not for speed, until it has.
fused = False
arith = 0

SIDE = 224                 # what Upsample(7) + AvgPool2d(S / 32) produce from S = 32 m
MAX_TOKENS = 64            # ide3d_vit_attention: T and the head dimension
MAX_HEAD_DIM = 64
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # CLIP's own normalisation of [0, 1] images, for `CLIPLoss(mean=, std=)`
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ---- the net (OpenAI CLIP, clip/model.py: QuickGELU, ResidualAttentionBlock, Transformer, VisionTransformer) ---------------------------------
class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class Attention(nn.Module):
    """`nn.MultiheadAttention(width, heads)` as CLIP calls it (self-attention, no mask, no dropout), with its parameter names:
    softmax_j((q_i / sqrt(d)) . k_j) v_j per head between `in_proj` and `out_proj`.  x: [n, T, C]."""

    def __init__(self, width, heads):
        super().__init__()
        assert width % heads == 0
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)

    def forward(self, x):
        n, T, C = x.shape
        d = C // self.heads
        q, k, v = (t.reshape(n, T, self.heads, d).transpose(1, 2) for t in F.linear(x, self.in_proj_weight, self.in_proj_bias).chunk(3, dim=-1))
        p = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2), dim=-1)
        return self.out_proj((p @ v).transpose(1, 2).reshape(n, T, C))


class ResidualAttentionBlock(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.attn = Attention(width, heads)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([('c_fc', nn.Linear(width, width * 4)), ('gelu', QuickGELU()), ('c_proj', nn.Linear(width * 4, width))]))
        self.ln_2 = nn.LayerNorm(width)

    def forward(self, x):
        x = x + self.attn(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class VisionTransformer(nn.Module):
    """CLIP's image tower: patch embedding (`conv1`, no bias), `class_embedding` in front, `positional_embedding` added, `ln_pre`, the
    blocks, `ln_post` on the class token, `@ proj` -> [n, output_dim].  `state_dict()` has the keys of CLIP's `visual` module.  The
    defaults are ViT-B/32; tests build narrow and shallow ones.  Randomly initialised (CLIP's own scales) until weights are loaded."""

    def __init__(self, input_resolution=224, patch_size=32, width=768, layers=12, heads=12, output_dim=512):
        super().__init__()
        assert input_resolution % patch_size == 0 and width % heads == 0
        self.input_resolution, self.patch_size, self.width, self.layers, self.heads, self.output_dim = input_resolution, patch_size, width, layers, heads, output_dim
        self.tokens = (input_resolution // patch_size) ** 2 + 1
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.tokens, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        proj_std, fc_std = scale * (2 * layers) ** -0.5, (2 * width) ** -0.5          # CLIP.initialize_parameters
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=scale)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)

    def forward(self, x):
        x = self.conv1(x)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)                                        # [n, g g, C]
        x = torch.cat([self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1), x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0, :]) @ self.proj

    def load_clip_state_dict(self, sd):
        """Load the image tower of a CLIP state dict: keys with or without the `visual.` prefix (other towers' entries are ignored), fp16
        or fp32 values.  Strict about the tower's own keys and shapes."""
        own = self.state_dict()
        has_prefix = any(k.startswith('visual.') for k in sd)
        picked = {}
        for k, v in sd.items():
            name = k[len('visual.'):] if k.startswith('visual.') else (None if has_prefix else k)
            if name in own:
                picked[name] = v.to(own[name].dtype)
        self.load_state_dict(picked, strict=True)
        return self

    @classmethod
    def from_clip_state_dict(cls, sd):
        """A net of the sizes a CLIP state dict's image tower has, with its weights."""
        sd = {(k[len('visual.'):] if k.startswith('visual.') else k): v for k, v in sd.items() if k.startswith('visual.') or not any(q.startswith('visual.') for q in sd)}
        width, _, patch, _ = sd['conv1.weight'].shape
        tokens = sd['positional_embedding'].shape[0]
        layers = len({k.split('.')[2] for k in sd if k.startswith('transformer.resblocks.')})
        net = cls(int(round(math.sqrt(tokens - 1))) * patch, patch, width, layers, max(width // 64, 1), sd['proj'].shape[1])
        return net.load_clip_state_dict(sd)


# ---- the fused pass, written against an `ops` object: `_HipOps` here, a float64 torch restatement in tests/clip_loss_ref.py --------------------
class _HipOps:
    """The launches of the fused pass.  conv: ide3d_modconv2d; residual_join, linear: csrc/res_join.hip, csrc/id_loss.hip; everything else:
    csrc/clip_loss.hip."""

    _instance = None

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    def __init__(self):
        from torch_utils import hip_plugin
        P, Q = hip_plugin.ClipLossPlugin, hip_plugin.IdLossPlugin
        self.prep, self.prep_backward, self.embed, self.embed_backward = P.prep, P.prep_backward, P.embed, P.embed_backward
        self.layernorm, self.layernorm_backward, self.attention, self.attention_backward = P.layernorm, P.layernorm_backward, P.attention, P.attention_backward
        self.quickgelu, self.quickgelu_backward, self.head, self.head_backward = P.quickgelu, P.quickgelu_backward, P.head, P.head_backward
        self.residual_join, self.linear, self.linear_backward_input = Q.residual_join, Q.linear, Q.linear_backward_input
        self._plan, self._factors = hip_plugin.modconv_plan, {}

    @staticmethod
    def conv(x, w, bias, relu, mode=0):
        return networks.plain_conv(x, w, bias, relu, mode, arith)

    def factor(self, n, cin, cout, T, bias):
        """(h, w) with h w = T for a dense product over T tokens: every factorisation is the same 1x1 convolution, so the one whose plan
        covers the fewest padded pixels is taken (ties: the fewest workgroups, then the widest rows)."""
        key = (n, cin, cout, T, bool(bias), arith)
        if key not in self._factors:
            best = None
            for h in range(1, T + 1):
                if T % h:
                    continue
                w = T // h
                info = self._plan(n, cin, cout, h, w, k=1, arith=arith, epilogue='bias' if bias else 'grad')
                tiles = -(-h // max(info['tile_h'], 1)) * -(-w // max(info['tile_w'], 1))
                cost = (tiles * info['tile_h'] * info['tile_w'], info['workgroups'], -w)
                if best is None or cost < best[0]:
                    best = (cost, (h, w))
            self._factors[key] = best[1]
        return self._factors[key]


def _w1x1(weight):
    """A dense layer's [cout, cin] weight (or the patch convolution's [C, 3, p, p]) as the [cout, cin, 1, 1] tensor the 1x1 launches
    read: one object per weight, so that the packed copy in the HIP workspace and the derived gradient weight stay valid."""
    return networks._wgrad_cache.get((weight,), lambda: weight.detach().reshape(weight.shape[0], -1, 1, 1), key='clip_1x1')


def _table(net):
    """[C, T]: positional_embedding^T with class_embedding added to column 0 (what ide3d_vit_embed adds to the patch tokens), cached."""
    def build():
        t = net.positional_embedding.detach().t().clone()
        t[:, 0] = net.class_embedding.detach() + net.positional_embedding.detach()[0]
        return t.contiguous()
    return networks._wgrad_cache.get((net.positional_embedding, net.class_embedding), build, key='clip_table')


def _proj_t(net):
    """proj^T [D, C]: the weight of the final projection as ide3d_linear reads it, cached."""
    return networks._wgrad_cache.get((net.proj,), lambda: net.proj.detach().t().contiguous(), key='clip_proj_t')


def _dense(ops, x, weight, bias=None):
    """x [n, cin, T] -> [n, cout, T] = weight x + bias per token: a 1x1 convolution over an h x w factorisation of T."""
    n, cin, T = x.shape
    w4 = _w1x1(weight)
    h, w = ops.factor(n, cin, w4.shape[0], T, bias is not None)
    return ops.conv(x.reshape(n, cin, h, w), w4, None if bias is None else bias.detach(), False).reshape(n, w4.shape[0], T)


def _dense_grad(ops, dy, weight):
    """The input gradient of `_dense`: the same launch on the transposed weight."""
    n, cout, T = dy.shape
    wg = networks._grad_weight(_w1x1(weight), True)
    h, w = ops.factor(n, cout, wg.shape[0], T, False)
    return ops.conv(dy.reshape(n, cout, h, w), wg, None, False).reshape(n, wg.shape[0], T)


def _ln(m):
    return m.weight.detach(), m.bias.detach()


def _fused_forward(ops, net, x, text, base, mean, std):
    """-> (out [n, T'] or None, avg [] = the mean of out or None, f [n, D], saved): x [n, 3, S, S]; text [T', D] or None (embeddings only); base
    [n, D] or None.  `saved` is what `_fused_backward` reads."""
    n, p, C = x.shape[0], net.patch_size, net.width
    patches = ops.conv(ops.prep(x, p, mean, std), _w1x1(net.conv1.weight), None, False)          # [n, C, g, g]
    table = _table(net)
    h, m0, r0 = ops.embed(patches, table, *_ln(net.ln_pre))                                      # [n, C, T]
    blocks = []
    for blk in net.transformer.resblocks:
        a, m1, r1 = ops.layernorm(h, *_ln(blk.ln_1))
        qkv = _dense(ops, a, blk.attn.in_proj_weight, blk.attn.in_proj_bias)
        h1 = ops.residual_join(h, _dense(ops, ops.attention(qkv, net.heads), blk.attn.out_proj.weight, blk.attn.out_proj.bias), 1.0)
        b, m2, r2 = ops.layernorm(h1, *_ln(blk.ln_2))
        u = _dense(ops, b, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
        h2 = ops.residual_join(h1, _dense(ops, ops.quickgelu(u), blk.mlp.c_proj.weight, blk.mlp.c_proj.bias), 1.0)
        blocks.append((blk, h, m1, r1, qkv, h1, m2, r2, u))
        h = h2
    cls, mp, rp = ops.layernorm(h, *_ln(net.ln_post), 1)                                          # the class token, [n, C, 1]
    f = ops.linear(cls.reshape(n, C), _proj_t(net))
    if text is None:
        return None, None, f, None
    out, e, norm, tnorm, avg = ops.head(f, text, base)
    return out, avg, f, dict(size=tuple(x.shape[2:]), std=std, patches=patches, m0=m0, r0=r0, blocks=blocks, top=h, mp=mp, rp=rp, e=e, norm=norm, tnorm=tnorm, text=text)


def _fused_backward(ops, net, sv, dout):
    """-> d (sum of out * dout) / d image.  dout: [n, T'] on the device."""
    n, C = sv['e'].shape[0], net.width
    df = ops.head_backward(sv['e'], sv['text'], sv['norm'], sv['tnorm'], dout)
    dcls = ops.linear_backward_input(df, _proj_t(net))
    dh = ops.layernorm_backward(dcls.reshape(n, C, 1), sv['top'], net.ln_post.weight.detach(), sv['mp'], sv['rp'])
    for blk, h, m1, r1, qkv, h1, m2, r2, u in reversed(sv['blocks']):
        du = ops.quickgelu_backward(_dense_grad(ops, dh, blk.mlp.c_proj.weight), u)
        dh1 = ops.layernorm_backward(_dense_grad(ops, du, blk.mlp.c_fc.weight), h1, blk.ln_2.weight.detach(), m2, r2, dh)          # + the skip's gradient
        dqkv = ops.attention_backward(qkv, _dense_grad(ops, dh1, blk.attn.out_proj.weight), net.heads)
        dh = ops.layernorm_backward(_dense_grad(ops, dqkv, blk.attn.in_proj_weight), h, blk.ln_1.weight.detach(), m1, r1, dh1)
    patches = sv['patches']
    dp = ops.embed_backward(dh, patches, _table(net), net.ln_pre.weight.detach(), sv['m0'], sv['r0'])
    dcol = ops.conv(dp, networks._grad_weight(_w1x1(net.conv1.weight), True), None, False)
    return ops.prep_backward(dcol, sv['size'], net.patch_size, sv['std'])


class _FusedClipLoss(torch.autograd.Function):
    """Embedding, 1 - cos against the text rows and the image gradient back through the net on the HIP entry points -> (out [n, T'],
    their mean, embeddings); `out` and the mean (summed in float64 by the head, rounded once) are differentiable, only with respect to the
    image; the backward is differentiable once.  The activations it keeps are the pass's own outputs, so they live on the context rather
    than in `save_for_backward`."""

    @staticmethod
    def forward(ctx, img, net, text, base, mean, std):
        out, avg, f, ctx.sv = _fused_forward(_HipOps.get(), net, img, text, base, mean, std)
        ctx.net = net
        ctx.mark_non_differentiable(f)
        return out, avg, f

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, davg, _df):
        dout = (dout + davg / dout.numel()).to(torch.float32).contiguous()          # [n, T']: the rows' own gradient + the mean's share
        return _fused_backward(_HipOps.get(), ctx.net, ctx.sv, dout), None, None, None, None, None


def _net_ok(net):
    """The limits of the HIP path on the net's sizes (host-side; the same on every device)."""
    if type(net) is not VisionTransformer or net.input_resolution != SIDE or SIDE % net.patch_size != 0:
        return False
    d = net.width // net.heads
    return net.tokens <= MAX_TOKENS and d % 4 == 0 and d <= MAX_HEAD_DIM and net.width % 4 == 0 and net.output_dim % 4 == 0


def _on_hip(net, img):
    if not (fused and isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.ndim == 4 and img.shape[1] == 3
            and img.shape[2] == img.shape[3] and img.shape[2] >= 32 and img.shape[2] % 32 == 0 and img.shape[2] <= 32 * 256
            and _net_ok(net) and not net.training):
        return False
    if any(p.requires_grad or p.dtype != torch.float32 or p.device != img.device for p in net.parameters()):
        return False
    return networks.use_hip_modconv and networks._modconv_init() and networks._modconv_grad_init()


def _rows(t, dev=None):
    """Text embeddings / a direction as detached float32 rows [T, D]."""
    t = t.detach()
    t = t[None] if t.ndim == 1 else t
    return t if dev is None else t.to(device=dev, dtype=torch.float32).contiguous()


class CLIPLoss(nn.Module):
    """`StyleCLIP/criteria/clip_loss.py::CLIPLoss` on text EMBEDDINGS, without the download: `.visual` is the ViT-B/32 image tower in eval
    mode, frozen.  Nothing is downloaded or loaded unless `weights` (a path or a state dict: CLIP's, or its `visual` module's) is given:
    WITHOUT LOADED WEIGHTS THE NET IS RANDOMLY INITIALISED.  The text encoder and its tokenizer stay the user's (see the module).
    `stylegan_size`: the generator's resolution as in the reference (any image whose side is a multiple of 32 is pooled by side // 32).
    `visual`: another `VisionTransformer` to use (tests build small ones).  `mean`, `std`: per-channel triples; when given, `preprocess`
    additionally applies ((x + 1) / 2 - mean) / std (`CLIP_MEAN`, `CLIP_STD`: CLIP's own); the default None is what StyleCLIP does."""

    def __init__(self, stylegan_size=512, visual=None, weights=None, mean=None, std=None):
        super().__init__()
        assert stylegan_size % 32 == 0 and (mean is None) == (std is None)
        self.stylegan_size = stylegan_size
        self.visual = visual if visual is not None else VisionTransformer()
        if weights is not None:
            self.visual.load_clip_state_dict(torch.load(weights, map_location='cpu') if isinstance(weights, (str, bytes)) or hasattr(weights, '__fspath__') else weights)
        self.upsample = nn.Upsample(scale_factor=7)
        self.avg_pool = nn.AvgPool2d(kernel_size=stylegan_size // 32)
        self.register_buffer('mean', None if mean is None else torch.tensor(mean, dtype=torch.float32).reshape(3))
        self.register_buffer('std', None if std is None else torch.tensor(std, dtype=torch.float32).reshape(3))
        self.visual.eval().requires_grad_(False)
        self.last_path = None

    def train(self, mode=True):
        """The image tower stays in eval mode (it is frozen)."""
        super().train(mode)
        self.visual.eval()
        return self

    def preprocess(self, image):
        """The reference's two lines (clip_loss.py:14): Upsample(7) then AvgPool2d(side // 32), + the normalisation when mean / std are set."""
        k = image.shape[-1] // 32
        x = (self.avg_pool if k == self.stylegan_size // 32 else nn.AvgPool2d(kernel_size=k))(self.upsample(image))
        if self.mean is not None:
            x = ((x + 1) / 2 - self.mean.to(x.dtype).reshape(1, 3, 1, 1)) / self.std.to(x.dtype).reshape(1, 3, 1, 1)
        return x

    def _definition(self, image):
        """The PyTorch definition, in the net's precision whatever the image's (an fp16 image is converted first, not pooled in fp16)."""
        return self.visual(self.preprocess(image.to(self.visual.conv1.weight.dtype)))

    def _hip(self, image):
        return _on_hip(self.visual, image) and (self.mean is None or (self.mean.device == image.device and self.mean.dtype == torch.float32))

    def features(self, image):
        """The embeddings [n, D] (not normalised).  Differentiable with respect to the image on the PyTorch path only; on the HIP path no
        gradient is recorded: use `forward` / `distance_to` / `directional` for one."""
        if self._hip(image) and not (torch.is_grad_enabled() and image.requires_grad):
            self.last_path = 'hip'
            with torch.no_grad():
                return _fused_forward(_HipOps.get(), self.visual, image.contiguous(), None, None, self.mean, self.std)[2]
        self.last_path = 'torch'
        return self._definition(image)

    def _cosine(self, image, text, base=None, mean=False):
        """-> [n, T] = 1 - cos(E(image) - base, text rows), or with `mean` their mean; the gradient flows to the image only on the HIP path."""
        if (self._hip(image) and not text.requires_grad and text.ndim in (1, 2) and text.shape[-1] == self.visual.output_dim
                and (base is None or (not base.requires_grad and tuple(base.shape) == (image.shape[0], self.visual.output_dim)))):
            self.last_path = 'hip'
            dev = image.device
            return _FusedClipLoss.apply(image.contiguous(), self.visual, _rows(text, dev), None if base is None else _rows(base, dev), self.mean, self.std)[1 if mean else 0]
        self.last_path = 'torch'
        f = self._definition(image)
        if base is not None:
            f = f - base.to(f.dtype)
        t = (text[None] if text.ndim == 1 else text).to(f.dtype)
        out = 1 - (f / f.norm(dim=1, keepdim=True)) @ (t / t.norm(dim=1, keepdim=True)).t()
        return out.mean() if mean else out

    def forward(self, image, text_features):
        """[n, T] = 1 - cos(E_img(image), text_features[t]): the reference's `1 - logits_per_image / 100` (clip_loss.py:15-16).
        text_features: [T, D] of any length (or [D])."""
        return self._cosine(image, text_features)

    def distance_to(self, image, text_features):
        """The mean of `forward`: the scalar of a training step."""
        return self._cosine(image, text_features, mean=True)

    def directional(self, image, source_features, direction):
        """mean(1 - cos(E(image) - source_features, direction)): the StyleGAN-NADA loss; source_features [n, D] = `features` of the frozen
        generator's images, direction [D] or [T, D] = the text direction (target - source text embeddings)."""
        return self._cosine(image, direction, source_features, mean=True)


def clip_distance(text_features, cliploss, weight=1.0, base=None):
    """The `distance` of `projection.project` that pulls the rendered image towards `text_features` ([T, D] or [D]): images (0..255) are
    mapped to -1..1 (`x / 127.5 - 1`) and the closure returns `weight * cliploss.distance_to(x, text_features)` (+ `base(images)` when
    given, e.g. `l2_distance(...)` or `lpips_distance(...)`)."""
    text = text_features.detach()

    def distance(images):
        d = weight * cliploss.distance_to(images / 127.5 - 1, text.to(images.device))
        return d + base(images) if base is not None else d
    return distance
