"""Depth-candidate correlation transformer (reference src/model/utils/{transformer.py:232-299,
encoder.py:13-209, attention.py:145-551, ffn.py:4-43}).

Module tree and parameter names match the reference (`encoder.layers.{i}.attentions.{j}.
{sampling_offsets,attention_weights,value_proj,output_proj}`, `ffns.0.layers.{0.0,1}`,
`norms.{0,1,2}`), so `depth_predictor.{coarse,fine}_transformer.*` checkpoint keys load.
Differences by design (MI355X):
  * the projection grid is never materialised: the correlation kernels recompute it from the
    cameras (`cameras=(intr, pose, disp)`), so `grid` is accepted for API parity but unused;
  * features stay channel-last [(b v), HW, C] throughout instead of the reference's
    [v, HW, b, C] permutations;
  * MSDA + correlation run fused on the GPU (kernels.uv_coarse / uv_cross / msda); the
    UVCoarseAttention.attention_weights Linear is kept for checkpoint parity but, as in the
    reference (softmax over one point == 1), does not affect the output.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from ... import kernels


# One split-bf16 GEMM where several nn.Linear modules read the same rows (the fine cross attention's
# sampling_offsets | attention_weights, both fine layers' value_proj); False = one GEMM per module
# (A/B scripts and the bit-identity test set it)
_MERGE_PROJ = True


def _split_cameras(cameras):
    """(intr, pose, disp, keywords) of a cameras tuple: its optional fourth element is
    kernels.pack_cameras(intr, pose) computed ahead (the depth predictor's camera prep), passed on to
    the device kernels as cams_packed (the CPU restatements of those ops do not take it)."""
    intr, pose, disp = cameras[:3]
    packed = cameras[3] if len(cameras) > 3 else None
    return intr, pose, disp, ({"cams_packed": packed} if packed is not None and packed.is_cuda else {})


def _cat_linears(owner, slot: str, linears):
    """(weight, bias) of several nn.Linear modules concatenated along the outputs, cached on `owner`
    per parameter version: one GEMM then serves every module that reads the same rows."""
    key = tuple((t.data_ptr(), t._version) for m in linears for t in (m.weight, m.bias))
    hit = owner.__dict__.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = (key, torch.cat([m.weight for m in linears], 0).contiguous(),
                   torch.cat([m.bias for m in linears], 0).contiguous())
        owner.__dict__[slot] = hit
    return hit[1], hit[2]


_REF2D: dict = {}  # (h, w, dtype, device) -> [1, h*w, 2] reference points
_WH: dict = {}     # (w, h, dtype, device) -> tensor([w, h])


class UVSelfAttention(nn.Module):
    """4-point deformable self-attention on the query grid (reference attention.py:145-277)."""

    def __init__(self, embed_dims=256, num_heads=1, num_levels=1, num_points=4, im2col_step=64, dropout=0.1,
                 batch_first=True):
        super().__init__()
        if num_heads != 1 or num_levels != 1:
            raise NotImplementedError("TranSplat uses one head and one level")
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)

    def core(self, query, value, query_pos, ref_2d, bev_h: int, bev_w: int):
        """The sampled values before output_proj (forward = output_proj(core) + identity)."""
        if query_pos is not None:
            query = query + query_pos
        bsv, nq, _ = query.shape
        value = self.value_proj(value)
        offsets = self.sampling_offsets(query).view(bsv, nq, self.num_points, 2)
        weights = self.attention_weights(query).view(bsv, nq, self.num_points).softmax(-1)
        # offset / (W, H) per coordinate (the reference divides by the spatial-shape tensor): one
        # broadcast division by a cached (W, H) tensor
        key = (bev_w, bev_h, offsets.dtype, str(offsets.device))
        wh = _WH.get(key)
        if wh is None:
            wh = _WH[key] = torch.tensor([bev_w, bev_h], dtype=offsets.dtype, device=offsets.device)
        loc = ref_2d[:, :, None, :] + offsets / wh
        return kernels.msda(value, loc, weights, bev_h, bev_w)

    def _proj_weights(self):
        """sampling_offsets and attention_weights as ONE [128, 2 C] linear on [query | query_pos]
        ((q + p) W^T = [q | p] [W | W]^T; rows 0-7 offsets, 8-11 logits, zero past them: the fused
        linear kernel's 128-wide output block), cached per parameter version."""
        so, aw = self.sampling_offsets, self.attention_weights
        key = tuple((t.data_ptr(), t._version) for t in (so.weight, so.bias, aw.weight, aw.bias))
        hit = self.__dict__.get("_pw")
        if hit is None or hit[0] != key:
            with torch.no_grad():
                w = torch.cat((so.weight, aw.weight), 0)
                b = torch.cat((so.bias, aw.bias), 0)
                wp = torch.zeros((128, 2 * w.shape[1]), dtype=torch.float32, device=w.device)
                wp[:w.shape[0], :w.shape[1]] = w
                wp[:w.shape[0], w.shape[1]:] = w
                bp = torch.zeros(128, dtype=torch.float32, device=w.device)
                bp[:b.shape[0]] = b
            hit = (key, wp, bp)
            self.__dict__["_pw"] = hit
        return hit[1], hit[2]

    def core_raw(self, query, value, query_pos, bev_h: int, bev_w: int):
        """core() with the position add and both projections as one fused linear launch and the
        softmax / offset scaling / reference points inside the sampling kernel (kernels.msda_raw):
        two launches instead of six. Needs the fp32 kernel path and query_pos."""
        wp, bp = self._proj_weights()
        ow = kernels.fused_linear(query, wp, x2=query_pos, bias=bp)
        value = self.value_proj(value)
        return kernels.msda_raw(value, ow.view(query.shape[0], query.shape[1], 128), self.num_points, bev_h, bev_w)

    def raw_ok(self, query, query_pos) -> bool:
        return (query_pos is not None and query.is_cuda and self.embed_dims <= 128
                and 3 * self.num_points <= 128 and query.dtype == torch.float32)

    def forward(self, query, value, query_pos, ref_2d, bev_h: int, bev_w: int):
        out = self.core(query, value, query_pos, ref_2d, bev_h, bev_w)
        return self.dropout(self.output_proj(out)) + query


class UVCrossAttention(nn.Module):
    """Per (pixel, depth) 4-point sampling of the other view, mean-correlated with the own
    feature (reference attention.py:279-416)."""

    def __init__(self, embed_dims=256, num_cams=1, dropout=0.1, bev_u=64, bev_v=64, batch_first=False):
        super().__init__()
        self.num_levels = 1
        self.num_heads = 1
        self.num_points = 4
        self.num_depth = 128
        self.dropout = nn.Dropout(dropout)
        self.embed_dims = embed_dims
        self.num_cams = num_cams
        n = num_cams * self.num_heads * self.num_levels * self.num_depth * self.num_points
        self.sampling_offsets = nn.Linear(embed_dims, n * 2)
        self.attention_weights = nn.Linear(embed_dims, n)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)

    def core(self, query, key_cl, value_cl, cameras, bev_h: int, bev_w: int, value=None):
        """The correlation before output_proj (forward = output_proj(core) + identity). value:
        value_proj(value_cl) where the caller already has it (UVTransformerEncoder computes the fine
        layers' projections of the shared features in one GEMM)."""
        if value is None:
            value = self.value_proj(value_cl)  # per view; the kernel reads the other view (the flip)
        so, aw = self.sampling_offsets, self.attention_weights
        if (_MERGE_PROJ and kernels.gemm_x3_takes(query, so.weight) and so.bias is not None
                and aw.bias is not None):
            # both projections of the same rows as one split-bf16 GEMM over [so.weight ; aw.weight];
            # the kernel reads the two column ranges of its output in place (the same bits as two GEMMs)
            w, b = _cat_linears(self, "_ow", (so, aw))
            ow = kernels.gemm_x3(query, w, b)
            offsets, logits = ow[..., :so.out_features], ow[..., so.out_features:]
        else:
            offsets = so(query)
            logits = aw(query)
        intr, pose, disp, kw = _split_cameras(cameras)
        return kernels.uv_cross(value, key_cl, intr, pose, disp, offsets, logits, bev_h, bev_w, **kw)

    def forward(self, query, key_cl, value_cl, cameras, bev_h: int, bev_w: int):
        out = self.core(query, key_cl, value_cl, cameras, bev_h, bev_w)
        return self.dropout(self.output_proj(out)) + query


class UVCoarseAttention(nn.Module):
    """Single-sample correlation per depth candidate (reference attention.py:418-551)."""

    def __init__(self, embed_dims=256, num_cams=1, dropout=0.1, bev_u=64, bev_v=64, batch_first=False):
        super().__init__()
        self.num_levels = 1
        self.num_heads = 1
        self.num_points = 1
        self.num_depth = 128
        self.embed_dims = embed_dims
        self.num_cams = num_cams
        self.attention_weights = nn.Linear(
            embed_dims, num_cams * self.num_heads * self.num_levels * self.num_depth * self.num_points)

    def forward(self, query, key_cl, cameras, bev_h: int, bev_w: int):
        """query None: the zero query the depth predictor starts from (the correlation as it is)."""
        intr, pose, disp, kw = _split_cameras(cameras)
        corr = kernels.uv_coarse(key_cl, intr, pose, disp, bev_h, bev_w, **kw)
        return corr if query is None else corr + query


class FFN(nn.Module):
    """Linear-ReLU-Linear with identity (reference ffn.py:4-43)."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.1, add_identity=True):
        super().__init__()
        self.embed_dims = embed_dims
        self.feedforward_channels = feedforward_channels
        self.activate = nn.ReLU(inplace=True)
        layers = []
        in_channels = embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(in_channels, feedforward_channels), self.activate,
                                        nn.Dropout(ffn_drop)))
            in_channels = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        out = self.layers(x)
        if not self.add_identity:
            return out
        return (x if identity is None else identity) + out


class UVTransformerEncoderLayer(nn.Module):
    """coarse: correlation only; fine: self-attn, LN, cross-attn, LN, FFN, LN
    (reference encoder.py:97-209)."""

    def __init__(self, embed_dims=256, num_haed=8, dropout=0.1, feedforward_channels=256, mode=None, with_cp=True):
        super().__init__()
        self.embed_dims = embed_dims
        self.mode = mode
        if mode == "coarse":
            self.attentions = nn.ModuleList([UVCoarseAttention(embed_dims=embed_dims)])
        elif mode == "fine":
            self.attentions = nn.ModuleList([UVSelfAttention(embed_dims=embed_dims),
                                             UVCrossAttention(embed_dims=embed_dims)])
            self.ffns = nn.ModuleList([FFN(embed_dims, feedforward_channels)])
            self.norms = nn.ModuleList([nn.LayerNorm(embed_dims) for _ in range(3)])
        else:
            raise NotImplementedError(mode)

    def forward(self, query, key_cl, bev_pos, ref_2d, cameras, bev_h, bev_w, value=None):
        if self.mode == "coarse":
            return self.attentions[0](query, key_cl, cameras, bev_h, bev_w)
        if self._fused_ok(query):
            return self._fine_fused(query, key_cl, bev_pos, ref_2d, cameras, bev_h, bev_w, value)
        if self._ln128_ok(query):  # bf16 dense mode: the post-norms as kernels (fp32 in and out)
            ln = lambda i, t: kernels.layer_norm128(t, self.norms[i], out_dtype=torch.float32)
        else:
            ln = lambda i, t: self.norms[i](t)
        query = ln(0, self.attentions[0](query, query, bev_pos, ref_2d, bev_h, bev_w))
        query = ln(1, self.attentions[1](query, key_cl, key_cl, cameras, bev_h, bev_w))
        return ln(2, self.ffns[0](query, None))

    def _ln128_ok(self, query) -> bool:
        return (self.embed_dims == 128 and query.is_cuda and torch.is_autocast_enabled(query.device.type)
                and torch.get_autocast_dtype(query.device.type) == torch.bfloat16)

    def _fused_ok(self, query) -> bool:
        ffn = self.ffns[0]
        return (query.dtype == torch.float32 and not torch.is_autocast_enabled(query.device.type)
                and self.embed_dims == 128 and len(ffn.layers) == 3 and ffn.feedforward_channels % 128 == 0)

    def _fine_fused(self, query, key_cl, bev_pos, ref_2d, cameras, bev_h, bev_w, value=None):
        """Fine layer with each output projection + bias + identity + LayerNorm (and the FFN's
        second Linear with its ReLU-on-load) as one kernels.fused_linear launch; same math as the
        module chain (dropout is the identity at test time)."""
        K = kernels
        sa, ca, ffn = self.attentions[0], self.attentions[1], self.ffns[0]
        ln = lambda m: (m.weight, m.bias, m.eps)
        if sa.raw_ok(query, bev_pos):
            out = sa.core_raw(query, query, bev_pos, bev_h, bev_w)
        else:
            out = sa.core(query, query, bev_pos, ref_2d, bev_h, bev_w)
        query = K.fused_linear(out, sa.output_proj.weight, bias=sa.output_proj.bias, ln=ln(self.norms[0]),
                               residual=query, res_pre_ln=True)
        out = ca.core(query, key_cl, key_cl, cameras, bev_h, bev_w, value=value)
        query = K.fused_linear(out, ca.output_proj.weight, bias=ca.output_proj.bias, ln=ln(self.norms[1]),
                               residual=query, res_pre_ln=True)
        fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
        hidden = K.fused_linear(query, fc1.weight, bias=fc1.bias)
        return K.fused_linear(hidden, fc2.weight, bias=fc2.bias, ln=ln(self.norms[2]), residual=query,
                              res_pre_ln=True, relu_in=True)


class UVTransformerEncoder(nn.Module):
    def __init__(self, num_layers=1, return_intermediate=False, embed_dims=256, mode=None):
        super().__init__()
        self.embed_dims = embed_dims
        self.num_layers = num_layers
        self.layers = nn.ModuleList([UVTransformerEncoderLayer(embed_dims, mode=mode) for _ in range(num_layers)])

    @staticmethod
    def reference_points_2d(bev_h, bev_w, n, dtype, device):
        """ref_2d pixel centres (i + 0.5) / size, (x, y) (reference encoder.py:61-71); a constant of
        the shape, built once per (shape, dtype, device) instead of ~7 launches per call."""
        key = (bev_h, bev_w, dtype, str(device))
        ref = _REF2D.get(key)
        if ref is None:
            ref_y, ref_x = torch.meshgrid(
                torch.linspace(0.5, bev_h - 0.5, bev_h, dtype=dtype, device=device),
                torch.linspace(0.5, bev_w - 0.5, bev_w, dtype=dtype, device=device), indexing="ij")
            ref = torch.stack((ref_x.reshape(-1) / bev_w, ref_y.reshape(-1) / bev_h), -1)[None]
            _REF2D[key] = ref
        return ref.expand(n, -1, -1)

    def _cross_values(self, query, key_cl):
        """value_proj(key_cl) of every fine layer's cross attention as one split-bf16 GEMM over the
        concatenated weights -> per layer a column range [..., 128] of its output (read in place by
        the correlation kernel), or None per layer where the layers run their own projection."""
        none = [None] * len(self.layers)
        if not _MERGE_PROJ or len(self.layers) < 2 or any(l.mode != "fine" or not l._fused_ok(query) for l in self.layers):
            return none
        projs = [l.attentions[1].value_proj for l in self.layers]
        if any(p.bias is None for p in projs) or not kernels.gemm_x3_takes(key_cl, projs[0].weight):
            return none
        w, b = _cat_linears(self, "_vw", projs)
        vals = kernels.gemm_x3(key_cl, w, b)
        c = projs[0].out_features
        return [vals[..., i * c:(i + 1) * c] for i in range(len(projs))]

    def forward(self, query, key_cl, bev_h, bev_w, bev_pos=None, cameras=None):
        # query, bev_pos: [(b v), HW, C]; key_cl: [B, 2, HW, C]; query None (coarse): a zero query
        n = key_cl.shape[0] * key_cl.shape[1] if query is None else query.shape[0]
        ref_2d = self.reference_points_2d(bev_h, bev_w, n, key_cl.dtype if query is None else query.dtype,
                                          key_cl.device)
        values = [None] * len(self.layers) if query is None else self._cross_values(query, key_cl)
        for layer, value in zip(self.layers, values):
            if value is None:
                query = layer(query, key_cl, bev_pos, ref_2d, cameras, bev_h, bev_w)
            else:
                query = layer(query, key_cl, bev_pos, ref_2d, cameras, bev_h, bev_w, value=value)
        return query


class UVTransformer(nn.Module):
    """(reference transformer.py:232-299) features [b, v, C, H, W] + queries -> correlation."""

    def __init__(self, embed_dims=256, num_layers=1, mode="coarse"):
        super().__init__()
        self.encoder = UVTransformerEncoder(embed_dims=embed_dims, mode=mode, num_layers=num_layers)
        self.embed_dims = embed_dims

    def forward(self, mlvl_feats, bev_queries, bev_u, bev_v, bev_pos=None, intrinsics=None, extrinsics=None,
                depth_sup=None, grid=None, depth=None, cameras=None, channel_last=None):
        """bev_queries / bev_pos: [(b v), HW, C] (channel-last, (b v) order); `cameras` =
        (pixel intrinsics [(v b),3,3], relative poses [(v b),4,4], disparities [(v b), D]).
        `channel_last` optionally passes the [b, 2, HW, C] view of mlvl_feats[0] precomputed."""
        if cameras is None:
            raise ValueError("UVTransformer needs cameras=(intr, pose, disp): the grid is computed in-kernel")
        feat = mlvl_feats[0]
        if channel_last is None:
            b, v, c, h, w = feat.shape
            channel_last = feat.flatten(3).transpose(2, 3).contiguous()  # [b, v, HW, C]
        return self.encoder(bev_queries, channel_last, bev_v, bev_u, bev_pos=bev_pos, cameras=cameras)
