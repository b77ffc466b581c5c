"""Test helpers for training/clip_loss.py: small image towers with seeded weights, a float64 functional restatement of the loss (independent
of the module: plain `torch.nn.functional` calls on a state dict), and `TorchOps`, a restatement in plain torch of every launch the fused
pass makes, so that `clip_loss._fused_forward` / `_fused_backward` - the orchestration the HIP path runs - can be checked against autograd
on the CPU, and each HIP pass against float64 on the GPU."""

import numpy as np
import torch
import torch.nn.functional as F

import parse_loss_ref

NARROW = dict(width=64, heads=2, layers=12, patch_size=32, output_dim=32)          # deep: twelve blocks of rounding on top of each other
WIDE = dict(width=768, heads=12, layers=2, patch_size=32, output_dim=512)          # ViT-B/32's widths: 50 tokens, head dimension 64
ODD = dict(width=60, heads=3, layers=2, patch_size=56, output_dim=20)              # 17 tokens, head dimension 20, widths that fill no tile
B16 = dict(width=64, heads=2, layers=1, patch_size=28, output_dim=32)              # 65 tokens: past what the HIP path covers
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def visual(spec, device='cpu', dtype=torch.float32, seed=5):
    """A `VisionTransformer` of `spec` with CLIP's initial scales, and biases and LayerNorm parameters that are not 0 and 1 (a dropped bias
    or gain must show)."""
    from training import clip_loss
    torch.manual_seed(seed)
    net = clip_loss.VisionTransformer(**spec)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('bias'):
                p.copy_(torch.rand(p.shape, generator=g) * 0.2 - 0.1)
            elif p.ndim == 1 and 'ln_' in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.6 + 0.7)
    return net.to(device=device, dtype=dtype).eval().requires_grad_(False)


def cliploss(spec, size, device='cpu', dtype=torch.float32, normalise=False):
    from training import clip_loss
    kw = dict(mean=CLIP_MEAN, std=CLIP_STD) if normalise else {}
    return clip_loss.CLIPLoss(stylegan_size=size, visual=visual(spec, device, dtype), **kw).to(device=device, dtype=dtype)


def images(shape, seed):
    """Images in -1..1: a smooth pattern plus noise, so that pooled windows differ and neighbours do not."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h) / h, torch.arange(w) / w, indexing='ij')
    base = torch.stack([torch.sin(6.0 * (yy * (1 + i) + xx * (2 - 0.5 * i)) + i) for i in range(n * c)]).reshape(n, c, h, w)
    return (0.6 * base + 0.4 * (torch.rand(shape, generator=g) * 2 - 1)).float()


def rows(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the loss from a state dict, functionally ----------------------------------------------------------------------------------------------------
def preprocess(x, mean=None, std=None):
    """The reference's two modules as functions: nearest up-sampling by 7, then average pooling by side // 32."""
    x = F.avg_pool2d(F.interpolate(x, scale_factor=7, mode='nearest'), x.shape[-1] // 32)
    if mean is not None:
        x = ((x + 1) / 2 - torch.as_tensor(mean, dtype=x.dtype, device=x.device).reshape(1, 3, 1, 1)) / torch.as_tensor(std, dtype=x.dtype, device=x.device).reshape(1, 3, 1, 1)
    return x


def _layer_norm(sd, p, x):
    return F.layer_norm(x, x.shape[-1:], sd[p + '.weight'], sd[p + '.bias'], 1e-5)


def embed(sd, x, heads, mean=None, std=None):
    """Embeddings [n, D] of images x in -1..1 from the state dict `sd`, in the dtype of both: token-major [n, T, C], F.multi_head_attention
    is not used - the attention is spelled out per head."""
    p = sd['conv1.weight'].shape[-1]
    x = F.conv2d(preprocess(x, mean, std), sd['conv1.weight'], stride=p).flatten(2).transpose(1, 2)
    n, _, C = x.shape
    x = torch.cat([sd['class_embedding'].expand(n, 1, C), x], dim=1) + sd['positional_embedding']
    x = _layer_norm(sd, 'ln_pre', x)
    d = C // heads
    i = 0
    while f'transformer.resblocks.{i}.ln_1.weight' in sd:
        b = f'transformer.resblocks.{i}.'
        q, k, v = F.linear(_layer_norm(sd, b + 'ln_1', x), sd[b + 'attn.in_proj_weight'], sd[b + 'attn.in_proj_bias']).split(C, dim=-1)
        outs = []
        for h in range(heads):
            s = slice(h * d, h * d + d)
            outs.append(torch.softmax(q[..., s] @ k[..., s].transpose(1, 2) / d ** 0.5, dim=-1) @ v[..., s])
        x = x + F.linear(torch.cat(outs, dim=-1), sd[b + 'attn.out_proj.weight'], sd[b + 'attn.out_proj.bias'])
        u = F.linear(_layer_norm(sd, b + 'ln_2', x), sd[b + 'mlp.c_fc.weight'], sd[b + 'mlp.c_fc.bias'])
        x = x + F.linear(u * torch.sigmoid(1.702 * u), sd[b + 'mlp.c_proj.weight'], sd[b + 'mlp.c_proj.bias'])
        i += 1
    return _layer_norm(sd, 'ln_post', x[:, 0]) @ sd['proj']


def cosine_rows(f, text, base=None):
    f = f if base is None else f - base
    text = text[None] if text.ndim == 1 else text
    return 1 - (f / f.norm(dim=1, keepdim=True)) @ (text / text.norm(dim=1, keepdim=True)).t()


def loss64(net, x, text, base=None, mean=None, std=None):
    """float64: (mean(1 - cos), d / d x, the [n, T] rows, the embeddings) of the restatement with the parameters of `net`."""
    sd = {k: v.double().cpu() for k, v in net.state_dict().items()}
    leaf = x.double().cpu().clone().requires_grad_(True)
    f = embed(sd, leaf, net.heads, mean, std)
    out = cosine_rows(f, text.double().cpu(), None if base is None else base.double().cpu())
    (g,) = torch.autograd.grad(out.mean(), [leaf])
    return float(out.mean().detach()), g, out.detach(), f.detach()


def _vjp(fn, x, dy):
    leaf = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


def unfold(x, p):
    """[n, 3, 224, 224] -> [n, 3 p p, g, g] in the channel order (ci p + ky) p + kx."""
    n, g = x.shape[0], x.shape[-1] // p
    return F.unfold(x, p, stride=p).reshape(n, 3 * p * p, g, g)


def prep_definition(x, p, mean=None, std=None):
    return unfold(preprocess(x, mean, std), p)


def embed_definition(patches, table, gamma, beta):
    """patches [n, C, ...] -> ln_pre over C of [class column | patches] + table -> [n, C, T]."""
    n, C = patches.shape[:2]
    tok = torch.cat([torch.zeros(n, C, 1, dtype=patches.dtype, device=patches.device), patches.reshape(n, C, -1)], dim=2) + table
    return layernorm_definition(tok, gamma, beta)


def layernorm_definition(x, gamma, beta, tokens=None):
    x = x if tokens is None else x[:, :, :tokens]
    return F.layer_norm(x.transpose(1, 2), x.shape[1:2], gamma, beta, 1e-5).transpose(1, 2)


def attention_definition(qkv, heads):
    n, C3, T = qkv.shape
    d = C3 // (3 * heads)
    q, k, v = (t.reshape(n, heads, d, T) for t in qkv.split(C3 // 3, dim=1))
    p = torch.softmax((q * d ** -0.5).transpose(2, 3) @ k, dim=-1)                        # [n, heads, T(i), T(j)]
    return (v @ p.transpose(2, 3)).reshape(n, C3 // 3, T)


def quickgelu_definition(x):
    return x * torch.sigmoid(1.702 * x)


class TorchOps(parse_loss_ref.TorchOps):
    """The `ops` of clip_loss._fused_forward / _fused_backward in torch, computing in `dtype` (conv: parse_loss_ref)."""

    @staticmethod
    def factor(n, cin, cout, T, bias):
        return 1, T

    def _c(self, t):
        return None if t is None else t.to(self.dtype)

    def prep(self, x, p, mean=None, std=None):
        return prep_definition(x.to(self.dtype), p, self._c(mean), self._c(std))

    def prep_backward(self, dcol, size, p, std=None):
        mean = None if std is None else torch.zeros_like(std)
        return _vjp(lambda t: self.prep(t, p, mean, std), torch.zeros(dcol.shape[0], 3, *size, dtype=dcol.dtype, device=dcol.device), dcol)

    @staticmethod
    def _stats(x):
        mean = x.mean(dim=1)
        return mean, (x.var(dim=1, unbiased=False) + 1e-5).rsqrt()

    def embed(self, patches, table, gamma, beta):
        n, C = patches.shape[:2]
        tok = torch.cat([torch.zeros(n, C, 1, dtype=patches.dtype, device=patches.device), patches.reshape(n, C, -1)], dim=2) + self._c(table)
        return (embed_definition(patches, self._c(table), self._c(gamma), self._c(beta)), *self._stats(tok))

    def embed_backward(self, dy, patches, table, gamma, mean, rstd):
        return _vjp(lambda t: embed_definition(t, self._c(table), self._c(gamma), torch.zeros_like(self._c(gamma))), patches, dy)

    def layernorm(self, x, gamma, beta, tokens=None):
        xs = x if tokens is None else x[:, :, :tokens]
        return (layernorm_definition(x, self._c(gamma), self._c(beta), tokens), *self._stats(xs))

    def layernorm_backward(self, dy, x, gamma, mean, rstd, add=None):
        g = _vjp(lambda t: layernorm_definition(t, self._c(gamma), torch.zeros_like(self._c(gamma)), dy.shape[2]), x, dy)
        return g if add is None else g + add

    @staticmethod
    def attention(qkv, heads):
        return attention_definition(qkv, heads)

    @staticmethod
    def attention_backward(qkv, dout, heads):
        return _vjp(lambda t: attention_definition(t, heads), qkv, dout)

    @staticmethod
    def quickgelu(x):
        return quickgelu_definition(x)

    @staticmethod
    def quickgelu_backward(dy, x):
        return _vjp(quickgelu_definition, x, dy)

    @staticmethod
    def residual_join(a, b, gain):
        return (a if b is None else a + b) * gain

    def linear(self, x, w, b=None):
        return F.linear(x.to(self.dtype), w.to(self.dtype), None if b is None else b.to(self.dtype))

    def linear_backward_input(self, dy, w):
        return dy.to(self.dtype) @ w.to(self.dtype)

    def head(self, f, text, base=None):
        v = f if base is None else f - self._c(base)
        norm, tnorm = v.norm(dim=1), self._c(text).norm(dim=1)
        e = v / norm[:, None]
        out = 1 - e @ (self._c(text) / tnorm[:, None]).t()
        return out, e, norm, tnorm, out.mean()

    def head_backward(self, e, text, norm, tnorm, dout):
        g = -dout.to(e.dtype) @ (self._c(text) / tnorm[:, None])
        return (g - e * (e * g).sum(1, keepdim=True)) / norm[:, None]


def ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))
