"""SAM half of the 2Haff hot path on MI355X: ViT image encoder, text-prompt encoder, left/right two-way mask
decoders and mask post-processing — host-side orchestration of the HIP kernels in csrc/ (no torch math).

Mirrors (same parameter names, same numerics contract) the reference's
  2Haff/model/segment_anything/modeling/image_encoder.py  (ImageEncoderViT.forward :110-125, Block :177-193)
  .../prompt_encoder.py (text path :140-186, get_dense_pe :67-76), .../mask_decoder.py (:79-178),
  .../transformer.py (:62-106,151-182), .../sam.py postprocess_masks (:155-189)
but batched over frames and prompts, channels-last everywhere, weights re-laid-out once at load time.
"""
import math

import torch

from . import ops

V = "model.visual_model"


def _f32(t, device):
    return t.to(device=device, dtype=torch.float32).contiguous()


class SamEncoderHip:
    """ImageEncoderViT: [B,3,S,S] normalised frames (or uint8 NHWC frames) -> [B, g*g, out_chans] channels-last."""

    def __init__(self, sd, cfg, dtype, device):
        s = self.cfg = cfg
        self.dtype, self.device = dtype, device
        E = V + ".image_encoder"
        C = s.embed_dim
        g = s.grid
        dev = device
        self.hd = C // s.heads
        self.w_patch = sd[E + ".patch_embed.proj.weight"].reshape(C, -1).to(dev, dtype).contiguous()
        self.b_patch = _f32(sd[E + ".patch_embed.proj.bias"], dev)
        self.pos = sd[E + ".pos_embed"].reshape(g * g, C).to(dev, dtype).contiguous()
        self.blocks = []
        # norm1 -> qkv and norm2 -> lin1 folded into the products (gamma into the weights, beta into the bias, per-row
        # {mean, rstd} from haff_row_stats applied in the GEMM epilogue: haff_gemm_bf16_ln). Default ON for the bf16 ViT-H
        # geometry since round 3 (the LayerNorm kernel's write + re-read of the normalised rows disappears: +0.5 % of the
        # step on the ring-loop GEMM, profiles/r3_fold_norms_ab.txt; it measured neutral on round 2's epilogue);
        # cfg.fold_norms = True / False forces it
        fold = getattr(cfg, "fold_norms", None)
        if fold is None:
            fold = dtype in (torch.bfloat16, torch.float16) and s.embed_dim == 1280 and s.window == 14
        fold = bool(fold) and dtype in (torch.bfloat16, torch.float16)   # (the fp16 mode follows the bf16 branches)
        for i in range(s.depth):
            B = f"{E}.blocks.{i}"
            is_global = i in s.global_idx
            S = g if is_global else s.window
            blk = {
                "global": is_global, "S": S,
                "n1w": _f32(sd[B + ".norm1.weight"], dev), "n1b": _f32(sd[B + ".norm1.bias"], dev),
                "wqkv": sd[B + ".attn.qkv.weight"].to(dev, dtype).contiguous(), "bqkv": _f32(sd[B + ".attn.qkv.bias"], dev),
                "wproj": sd[B + ".attn.proj.weight"].to(dev, dtype).contiguous(), "bproj": _f32(sd[B + ".attn.proj.bias"], dev),
                "rel_h": _f32(self._fit_rel_pos(sd[B + ".attn.rel_pos_h"], S), dev),
                "rel_w": _f32(self._fit_rel_pos(sd[B + ".attn.rel_pos_w"], S), dev),
                "n2w": _f32(sd[B + ".norm2.weight"], dev), "n2b": _f32(sd[B + ".norm2.bias"], dev),
                "w1": sd[B + ".mlp.lin1.weight"].to(dev, dtype).contiguous(), "b1": _f32(sd[B + ".mlp.lin1.bias"], dev),
                "w2": sd[B + ".mlp.lin2.weight"].to(dev, dtype).contiguous(), "b2": _f32(sd[B + ".mlp.lin2.bias"], dev),
            }
            if fold:
                blk["wqkv_f"], blk["sqkv"], blk["bqkv_f"] = ops.fold_norm(blk["wqkv"], blk["n1w"], blk["n1b"], blk["bqkv"], dtype)
                blk["w1_f"], blk["s1"], blk["b1_f"] = ops.fold_norm(blk["w1"], blk["n2w"], blk["n2b"], blk["b1"], dtype)
            self.blocks.append(blk)
        self.w_neck0 = sd[E + ".neck.0.weight"].reshape(s.out_chans, C).to(dev, dtype).contiguous()
        self.neck1 = (_f32(sd[E + ".neck.1.weight"], dev), _f32(sd[E + ".neck.1.bias"], dev))
        # 3x3 conv as GEMM over (ky, kx, cin) columns — matches haff_im2col3x3
        self.w_neck2 = sd[E + ".neck.2.weight"].permute(0, 2, 3, 1).reshape(s.out_chans, -1).to(dev, dtype).contiguous()
        self.neck3 = (_f32(sd[E + ".neck.3.weight"], dev), _f32(sd[E + ".neck.3.bias"], dev))
        self._maps = {}
        self.fold_norms = fold        # (see above; False = the LayerNorm kernels, needs no other change)
        self.compact_windows = True   # windowed blocks skip the padded window rows (bf16, ViT-H window geometry)
        # ... and their q|k|v product scatters HEAD-MAJOR ([q|k|v][window][head][token][80]: haff_gemm_bf16_heads), so that an
        # item's K and V are one contiguous 31 KB block each for the window kernel's staging DMA (round 5; token-major rows are
        # 160-B pieces at a 7680-B stride). False: the token-major [window token][3 * C] buffer of rounds 1-4.
        self.head_major_windows = True
        self.fused_global = True      # global blocks: rel-pos inside the attention kernel (bf16, ViT-H geometry); False = tables
        self.producer_stats = True    # folded norms: row statistics from the producing product's epilogue (batches whose proj /
        #                               lin2 run on the 8-wave tile anyway: >= 2 frames; "force": any); False = haff_row_stats
        # fp32 image embeddings out of the neck (bf16 mode): the last 3x3-conv GEMM writes its fp32 accumulators and the
        # final LayerNorm2d runs in fp32, so the decoder tail (LisaMI355.fp32_tail) starts from un-rounded embeddings.
        # One bf16 rounding of the embedding ALONE costs 0.0005-0.0014 of mask IoU on random weights (tools/parity_sim.py).
        self.emb_f32 = False
        # fp32 RESIDUAL STREAM (bf16 mode; round 5): the stream x lives in HBM as fp32 — proj / lin2 add
        # their fp32 accumulators to it and write fp32 back, LayerNorm reads it and hands ONE bf16 rounding of the NORMALISED row
        # to the bf16 MFMA products — so the 64 per-block roundings of the stream itself (the dominant term of the bf16 mode's
        # distance to the reference at depth 32: tools/full_frame_parity.py) disappear. Costs the folded norms (LayerNorm kernels
        # come back) and doubles the epilogue traffic of proj / lin2. Off by default.
        self.fp32_stream = False
        # ... round 6: the FUSED form — the proj / lin2 epilogue writes the fp32 stream AND its bf16 copy (haff_gemm_bf16_rowstats32),
        # the norms stay folded (their operand is the copy); taken whenever fp32_stream is on and the shapes allow (ViT-H geometry,
        # >= 2 frames per pass). False: round 5's unfused form everywhere (A/B).
        self.fused_fp32_stream = True
        # the neck on the f32-input MFMA path (bf16 mode): see forward_rows
        self.neck_f32 = dtype == torch.float16   # fp16: always (the reference's own overflow guard, image_encoder.py:118-124)
        self._neck32 = None
        self._pos32 = None

    @staticmethod
    def _fit_rel_pos(table, S):
        """get_rel_pos's interpolation branch (image_encoder.py:333-344); a no-op for SAM checkpoints."""
        L = 2 * S - 1
        if table.shape[0] == L:
            return table
        t = torch.nn.functional.interpolate(table.float().reshape(1, table.shape[0], -1).permute(0, 2, 1), size=L, mode="linear")
        return t.reshape(-1, L).permute(1, 0)

    def _window_maps(self, B):
        """Gather map (window row -> image token row, -1 = zero pad) used both ways (image_encoder.py:263-318)."""
        if B in self._maps:
            return self._maps[B]
        s = self.cfg
        g, ws = s.grid, s.window
        gp = (g + ws - 1) // ws * ws
        nw = gp // ws
        idx = torch.full((B, gp, gp), -1, dtype=torch.int64)
        base = torch.arange(g * g).view(g, g)
        for b in range(B):
            idx[b, :g, :g] = base + b * g * g
        win = idx.view(B, nw, ws, nw, ws).permute(0, 1, 3, 2, 4).reshape(-1).to(torch.int32).to(self.device)
        self._maps[B] = (win, nw * nw)
        return self._maps[B]

    def _compact_window_map(self, B):
        """Inverse of _window_maps: image token row -> its row in the window-major padded layout (int32 [B*g*g])."""
        key = ("inv", B)
        if key not in self._maps:
            win, _ = self._window_maps(B)
            valid = win >= 0
            inv = torch.empty((B * self.cfg.grid * self.cfg.grid,), dtype=torch.int32, device=self.device)
            inv[win[valid].long()] = torch.arange(win.numel(), dtype=torch.int32, device=self.device)[valid]
            self._maps[key] = inv
        return self._maps[key]

    def _head_major_window_map(self, B):
        """image token row -> window * heads * n_tok + token-in-window (int32 [B*g*g]): the row part of the head-major q|k|v
        scatter (ops.linear_heads), in units of one head's token row."""
        key = ("hm", B)
        if key not in self._maps:
            inv = self._compact_window_map(B).long()
            ntok = self.cfg.window * self.cfg.window
            self._maps[key] = ((inv // ntok) * (self.cfg.heads * ntok) + inv % ntok).to(torch.int32)
        return self._maps[key]

    def _windowed_qkv(self, x, blk, B, st, folded):
        """q, k, v views [windows, heads, tokens, d] of one windowed block's projection of the REAL tokens + the pad-token row index
        the window kernel substitutes for padded window positions. Head-major planes when the shapes allow, else token-major."""
        s = self.cfg
        C, H, hd = s.embed_dim, s.heads, self.hd
        _, nw2 = self._window_maps(B)
        nb, ntok = B * nw2, s.window * s.window
        w, bias = (blk["wqkv_f"], blk["bqkv_f"]) if folded else (blk["wqkv"], blk["bqkv"])
        kw = dict(ln_stats=st, ln_colsum=blk["sqkv"]) if folded else {}
        part = (nb + 1) * H * ntok * hd
        # (the window kernel reaches V's pad row through one 32-bit byte offset of ~ 2 planes: 2 * part * 2 bytes must stay under
        # 4 GiB — passes of > 170 frames keep the token-major buffer; haff_window_attention_bf16 refuses the wrap either way)
        if self.head_major_windows and ops.linear_heads_supported(x.shape[0], 3 * C, C, hd, H, x.dtype) and 4 * part + 4 * hd < (1 << 32):
            planes = torch.empty((3, nb + 1, H, ntok, hd), dtype=x.dtype, device=x.device)
            ops.linear_heads(x, w, bias, self._head_major_window_map(B), planes, hd, H, part, ntok * hd, **kw)
            planes[:, nb, :, 0, :].copy_(blk["bqkv"].view(3, H, hd))   # the pad token: qkv of a zero row = the bias
            return planes[0, :nb], planes[1, :nb], planes[2, :nb], nb * H * ntok
        qkv = torch.empty((nb * ntok + 1, 3 * C), dtype=x.dtype, device=x.device)
        ops.linear(x, w, bias=bias, row_map=self._compact_window_map(B), out=qkv[:-1], **kw)
        qkv[-1].copy_(blk["bqkv"])
        q5 = qkv[:-1].view(nb, ntok, 3, H, hd)
        return q5[:, :, 0].permute(0, 2, 1, 3), q5[:, :, 1].permute(0, 2, 1, 3), q5[:, :, 2].permute(0, 2, 1, 3), nb * ntok

    def patch_rows_from_nchw(self, images):
        s = self.cfg
        return ops.patchify_nchw(images, s.patch, s.grid, s.grid, 3 * s.patch * s.patch, self.dtype)

    def patch_rows_from_u8(self, frames, mean, std):
        s = self.cfg
        return ops.patchify_u8(frames, s.patch, s.grid, s.grid, 3 * s.patch * s.patch, mean, std, self.dtype)

    def forward_rows(self, rows, B, taps=None, out=None):
        """Patch rows -> image embedding [B, N, out_chans] (image_encoder.py:110-125,177-193). One body for the three forms of the
        residual stream x [B*N, C]:
          bf16 (default)     x is bf16; proj / lin2 add into it (and, when the shapes allow, emit the LayerNorm statistics of the
                             rows they wrote); norm1 -> qkv and norm2 -> lin1 are folded into the products.
          fp32, fused        (fp32_stream, round 6) x is fp32 and x16 its bf16 copy, BOTH written by the proj / lin2 epilogue
                             (ops.linear_rowstats32): the stream is never rounded between blocks, the folded norms stay, the
                             products' operand is one rounding of the stream.
          fp32, unfused      (fp32_stream where the fused form's shapes are not met, or fused_fp32_stream = False: round 5's form)
                             LayerNorm kernels read fp32 and round the NORMALISED row to bf16; proj / lin2 take and write fp32."""
        s = self.cfg
        C, g, H, hd = s.embed_dim, s.grid, s.heads, self.hd
        N = g * g
        bf = torch.bfloat16
        s32 = bool(self.fp32_stream) and self.dtype == bf
        if s32:
            if self._pos32 is None:
                self._pos32 = self.pos.float()
            x = ops.linear(rows, self.w_patch, bias=self.b_patch, out_dtype=torch.float32)
            x = ops.add_bcast(x, self._pos32, mod=N, out=x)
        else:
            x = ops.linear(rows, self.w_patch, bias=self.b_patch)
            x = ops.add_bcast(x, self.pos, mod=N, out=x)
        scale = hd ** -0.5
        compact_ok = self.compact_windows and self.dtype in (bf, torch.float16) and s.window == 14 and hd == 80
        # folded norms: {mean, rstd} of the rows of x, handed from the product that WROTE x (proj / lin2 epilogues sum their own
        # results: ops.linear_rowstats) to the product that normalises it; None = take a statistics pass (ops.row_stats)
        carry = self.fold_norms and self.producer_stats and \
            ops.linear_rowstats_supported(x.shape[0], C, C, self.dtype, 0 if self.producer_stats == "force" else 160)
        fused32 = s32 and self.fused_fp32_stream and carry and compact_ok    # (every residual product then has whole rows, no row map)
        fold = self.fold_norms and (not s32 or fused32)
        x16 = x.to(bf) if fused32 else None       # the products' operand: the stream rounded once (kept up to date by the epilogues)
        nkw = {"out_dtype": bf} if s32 else {}
        st = None

        def stats():
            return st if st is not None else ops.row_stats(x, 1e-6)

        def add_product(a2, w, b, a_map=None, row_map=None):
            """x += a2 @ w.T + b (image_encoder.py:186-188 / :193); returns the statistics of the new rows or None."""
            if fused32:
                return ops.linear_rowstats32(a2, w, b, x, x16, 1e-6, a_map=a_map)
            if carry and row_map is None and not s32:
                return ops.linear_rowstats(a2, w, b, x, 1e-6, out=x, a_map=a_map)[1]
            ops.linear(a2, w, bias=b, resid=x, a_map=a_map, row_map=row_map, out=x)
            return None
        for i, blk in enumerate(self.blocks):
            xa = x16 if fused32 else x
            if compact_ok and not blk["global"]:
                # Windowed block, real tokens only: the padded window rows (16 % of the rows at 64x64 / 14) are never
                # normalised, projected or written. qkv rows are scattered straight into the window-major layout;
                # the fused window kernel substitutes the one "pad token" row (qkv of a zero token = the bias, since
                # window_partition pads AFTER norm1, image_encoder.py:179-183) for them; proj gathers the real rows
                # back (window_unpartition drops the pads right after, :186-188).
                _, nw2 = self._window_maps(B)
                inv = self._compact_window_map(B)
                nb, ntok, S = B * nw2, s.window * s.window, s.window
                if fold:
                    q, k, v, pad = self._windowed_qkv(xa, blk, B, stats(), True)
                else:
                    q, k, v, pad = self._windowed_qkv(ops.layernorm(x, blk["n1w"], blk["n1b"], 1e-6, **nkw), blk, B, None, False)
                a = ops.window_attention(q, k, v, scale, blk["rel_h"], blk["rel_w"], S, grid=g, pad_token=pad)
                del q, k, v
                st = add_product(a.view(nb * ntok, C), blk["wproj"], blk["bproj"], a_map=inv)
            else:
                if blk["global"]:
                    nb, ntok, S, row_map = B, N, g, None
                    if fold:
                        qkv = ops.linear(xa, blk["wqkv_f"], bias=blk["bqkv_f"], ln_stats=stats(), ln_colsum=blk["sqkv"])
                    else:
                        qkv = ops.linear(ops.layernorm(x, blk["n1w"], blk["n1b"], 1e-6, **nkw), blk["wqkv"], bias=blk["bqkv"])
                else:
                    win, nw2 = self._window_maps(B)
                    xn = ops.layernorm(x, blk["n1w"], blk["n1b"], 1e-6, in_map=win, **nkw)
                    nb, ntok, S, row_map = B * nw2, s.window * s.window, s.window, win
                    qkv = ops.linear(xn, blk["wqkv"], bias=blk["bqkv"])
                q5 = qkv.view(nb, ntok, 3, H, hd)
                q = q5[:, :, 0].permute(0, 2, 1, 3)
                k = q5[:, :, 1].permute(0, 2, 1, 3)
                v = q5[:, :, 2].permute(0, 2, 1, 3)
                if not blk["global"] and ops.window_attention_supported(q, S):
                    a = ops.window_attention(q, k, v, scale, blk["rel_h"], blk["rel_w"], S)
                elif blk["global"] and self.fused_global and ops.global_attention_supported(q, k, v, S):
                    a = ops.global_attention(q, k, v, scale, blk["rel_h"], blk["rel_w"], S)
                else:
                    relh, relw = ops.relpos_tables(q, blk["rel_h"], blk["rel_w"], S)
                    a = ops.attention(q, k, v, scale, relh=relh, relw=relw, S=S)
                    del relh, relw
                del qkv
                st = add_product(a.view(nb * ntok, C), blk["wproj"], blk["bproj"], row_map=row_map)
            if fold:
                h = ops.linear(x16 if fused32 else x, blk["w1_f"], bias=blk["b1_f"], act=ops.ACT_GELU, ln_stats=stats(), ln_colsum=blk["s1"])
            else:
                h = ops.layernorm(x, blk["n2w"], blk["n2b"], 1e-6, **nkw)
                h = ops.linear(h, blk["w1"], bias=blk["b1"], act=ops.ACT_GELU)
            st = add_product(h, blk["w2"], blk["b2"])
            if taps is not None:
                taps[f"block{i}"] = x.float().view(B, g, g, C).cpu()
        o = None if out is None else out.view(B * N, s.out_chans)
        if self.neck_f32 and self.dtype in (bf, torch.float16):
            # the neck (image_encoder.py:88-107: 1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d) on the f32-input MFMA path: its four
            # tensors are the last roundings in front of the embedding and nothing averages them out afterwards; 7.5 GFLOP per frame
            if self._neck32 is None:
                self._neck32 = (self.w_neck0.float(), self.w_neck2.float())
            y = ops.linear(x if s32 else x.float(), self._neck32[0])
            y = ops.layernorm(y, self.neck1[0], self.neck1[1], 1e-6)
            cols = ops.im2col3x3(y.view(B, g, g, s.out_chans))
            y = ops.linear(cols, self._neck32[1])
            if not self.emb_f32:
                return ops.layernorm(y, self.neck3[0], self.neck3[1], 1e-6, out=o, out_dtype=self.dtype).view(B, N, s.out_chans)
            return ops.layernorm(y, self.neck3[0], self.neck3[1], 1e-6, out=o).view(B, N, s.out_chans)
        y = ops.linear(x16 if fused32 else (x.to(bf) if s32 else x), self.w_neck0)
        y = ops.layernorm(y, self.neck1[0], self.neck1[1], 1e-6)
        cols = ops.im2col3x3(y.view(B, g, g, s.out_chans))
        y = ops.linear(cols, self.w_neck2, out_dtype=torch.float32 if self.emb_f32 else None)
        # (out: a [B, N, out_chans] slice of the caller's embedding buffer — several passes fill one tensor, no torch.cat)
        y = ops.layernorm(y, self.neck3[0], self.neck3[1], 1e-6, out=o)
        return y.view(B, N, s.out_chans)

    def __call__(self, images, taps=None):
        """images [B,3,S,S] already normalised/padded (the evaluate() contract, LISA.py:487)."""
        images = images.to(self.dtype)
        return self.forward_rows(self.patch_rows_from_nchw(images), images.shape[0], taps)


class SamDecoderSideHip:
    """One MaskDecoder (left: taxonomy head on; right: off), batched over prompts."""

    def __init__(self, sd, pfx, cfg, dtype, device, taxonomy_on):
        self.dtype, self.device, self.taxonomy_on = dtype, device, taxonomy_on
        self.C = C = cfg.out_chans
        dev = device

        def lin(name):
            return sd[name + ".weight"].to(dev, dtype).contiguous(), _f32(sd[name + ".bias"], dev)

        def norm(name):
            return _f32(sd[name + ".weight"], dev), _f32(sd[name + ".bias"], dev)

        def attn(name):
            return {n: lin(f"{name}.{n}_proj") for n in ("q", "k", "v", "out")}
        self.out_tokens = torch.cat([sd[pfx + ".iou_token.weight"], sd[pfx + ".mask_tokens.weight"]], 0).to(dev, dtype)
        T = pfx + ".transformer"
        self.layers = []
        for l in range(2):
            L = f"{T}.layers.{l}"
            self.layers.append({
                "self": attn(L + ".self_attn"), "t2i": attn(L + ".cross_attn_token_to_image"),
                "i2t": attn(L + ".cross_attn_image_to_token"),
                "n1": norm(L + ".norm1"), "n2": norm(L + ".norm2"), "n3": norm(L + ".norm3"), "n4": norm(L + ".norm4"),
                "lin1": lin(L + ".mlp.lin1"), "lin2": lin(L + ".mlp.lin2")})
        self.final = attn(T + ".final_attn_token_to_image")
        self.nf = norm(T + ".norm_final_attn")
        # ConvTranspose2d(C -> C/4, k2 s2) as a per-pixel GEMM: output column (dy*2+dx)*C/4 + co
        w = sd[pfx + ".output_upscaling.0.weight"]  # [ci, co, dy, dx]
        self.w_up1 = w.permute(2, 3, 1, 0).reshape(4 * (C // 4), C).to(dev, dtype).contiguous()
        self.b_up1 = _f32(sd[pfx + ".output_upscaling.0.bias"].repeat(4), dev)
        self.ln_up = norm(pfx + ".output_upscaling.1")
        w = sd[pfx + ".output_upscaling.3.weight"]  # [co, c2, dy2, dx2] -> [co][(dy2,dx2,c2)]
        self.w_up2 = _f32(w.permute(0, 2, 3, 1).reshape(C // 4, 4 * (C // 8)), dev)
        self.b_up2 = _f32(sd[pfx + ".output_upscaling.3.bias"], dev)
        self.hyper = [[lin(f"{pfx}.output_hypernetworks_mlps.{i}.layers.{j}") for j in range(3)] for i in range(4)]
        self.iou_head = [lin(f"{pfx}.iou_prediction_head.layers.{j}") for j in range(3)]
        if taxonomy_on:
            self.tax = [lin(f"{pfx}.taxonomy_embed.layers.{j}") for j in range(3)]

    def _attend(self, w, q_in, k_in, v_in, P, nq, nk, heads=8):
        qp = ops.linear(q_in, *w["q"])
        kp = ops.linear(k_in, *w["k"])
        vp = ops.linear(v_in, *w["v"])
        d = qp.shape[1] // heads
        q = qp.view(P, nq, heads, d).permute(0, 2, 1, 3)
        k = kp.view(P, nk, heads, d).permute(0, 2, 1, 3)
        v = vp.view(P, nk, heads, d).permute(0, 2, 1, 3)
        a = ops.attention(q, k, v, 1.0 / math.sqrt(d))
        return a.view(P * nq, heads * d), w["out"]

    def _mlp3(self, layers, x, last_f32=True):
        x = ops.linear(x, *layers[0], act=ops.ACT_RELU)
        x = ops.linear(x, *layers[1], act=ops.ACT_RELU)
        return ops.linear(x, *layers[2], out_dtype=torch.float32 if last_f32 else None)

    def __call__(self, src, key_pe, text, grid, taps=None):
        """src [P, N, C] (image embedding + dense prompt), key_pe [N, C], text [P, C] -> low-res logits [P,4g,4g]."""
        P, N, C = src.shape
        nt = 6
        tokens = torch.cat([self.out_tokens.unsqueeze(0).expand(P, -1, -1), text.view(P, 1, C).to(self.dtype)], dim=1)
        tokens = tokens.contiguous().view(P * nt, C)
        queries = tokens
        keys = src.reshape(P * N, C)
        for li, L in enumerate(self.layers):
            if li == 0:
                a, wo = self._attend(L["self"], queries, queries, queries, P, nt, nt)
                queries = ops.linear(a, *wo)
            else:
                q = ops.add_bcast(queries, tokens)
                a, wo = self._attend(L["self"], q, q, queries, P, nt, nt)
                queries = ops.linear(a, *wo, resid=queries)
            queries = ops.layernorm(queries, *L["n1"], 1e-5)
            q = ops.add_bcast(queries, tokens)
            k = ops.add_bcast(keys, key_pe, mod=N)
            a, wo = self._attend(L["t2i"], q, k, keys, P, nt, N)
            queries = ops.layernorm(ops.linear(a, *wo, resid=queries), *L["n2"], 1e-5)
            h = ops.linear(queries, *L["lin1"], act=ops.ACT_RELU)
            queries = ops.layernorm(ops.linear(h, *L["lin2"], resid=queries), *L["n3"], 1e-5)
            q = ops.add_bcast(queries, tokens)
            a, wo = self._attend(L["i2t"], k, q, queries, P, N, nt)
            keys = ops.layernorm(ops.linear(a, *wo, resid=keys), *L["n4"], 1e-5)
            if taps is not None:
                taps[f"layer{li}.queries"] = queries.float().view(P, nt, C).cpu()
                taps[f"layer{li}.keys"] = keys.float().view(P, N, C).cpu()
        q = ops.add_bcast(queries, tokens)
        k = ops.add_bcast(keys, key_pe, mod=N)
        a, wo = self._attend(self.final, q, k, keys, P, nt, N)
        queries = ops.layernorm(ops.linear(a, *wo, resid=queries), *self.nf, 1e-5)
        hs = queries.view(P, nt, C)
        up1 = ops.linear(keys, self.w_up1, bias=self.b_up1)
        hyper0 = self._mlp3(self.hyper[0], hs[:, 1])
        low_res = ops.upscale_mask(up1, self.ln_up[0], self.ln_up[1], self.w_up2, self.b_up2, hyper0, P, grid, grid)
        iou = self._mlp3(self.iou_head, hs[:, 0])[:, 0:1]
        tax = None
        if self.taxonomy_on:
            tax = ops.softmax_rows(self._mlp3(self.tax, hs[:, 1:5].reshape(P, 4 * C)).contiguous())
        return low_res, iou, tax


class SamPromptDecoderHip:
    """PromptEncoder text path + both decoders + postprocess (LISA.py:494-532), batched over all prompts."""

    def __init__(self, sd, cfg, dtype, device):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        P = V + ".prompt_encoder"
        g = cfg.grid
        C = cfg.out_chans
        # dense PE is input-independent: compute once (prompt_encoder.py:203-229), x first then y
        G = sd[P + ".pe_layer.positional_encoding_gaussian_matrix"].float().cpu()
        ys = (torch.arange(g, dtype=torch.float32) + 0.5) / g
        xs = (torch.arange(g, dtype=torch.float32) + 0.5) / g
        coords = torch.stack([xs[None, :].expand(g, g), ys[:, None].expand(g, g)], dim=-1)
        c = 2 * math.pi * ((2 * coords - 1) @ G)
        self.key_pe = torch.cat([torch.sin(c), torch.cos(c)], dim=-1).reshape(g * g, C).to(device, dtype).contiguous()
        self.no_mask = sd[P + ".no_mask_embed.weight"].reshape(1, C).to(device, dtype).contiguous()
        self.left = SamDecoderSideHip(sd, V + ".mask_decoder_left", cfg, dtype, device, True)
        self.right = SamDecoderSideHip(sd, V + ".mask_decoder_right", cfg, dtype, device, False)
        # a handful of prompts: the two decoders are two independent chains of ~70 latency-bound launches each; they run
        # side by side on two HIP streams (inside the tail's hipGraph: two parallel branches) — at every prompt count (round 5).
        self.pair_streams = True
        self.pair_max_prompts = 1 << 30   # (rounds 1-4: 8 — "many prompts fill the chip"; but at 64 prompts the TOKEN-side products
                                          # are still 8-workgroup latency chains of 33 us each: side by side +0.4 % of the 64-frame step)
        self._pair_stream = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None

    def decode(self, emb, frame_idx, text, taps=None):
        """emb [Bf, N, C]; frame_idx int64 [P] (prompt -> frame); text [P, C]."""
        P = text.shape[0]
        N, C = emb.shape[1], emb.shape[2]
        src = emb.index_select(0, frame_idx).reshape(P * N, C).to(self.dtype)
        src = ops.add_bcast(src, self.no_mask, mod=1).view(P, N, C)
        if self.pair_streams and self._pair_stream is not None and P <= self.pair_max_prompts and taps is None:
            cur, side = torch.cuda.current_stream(self.device), self._pair_stream
            capturing = torch.cuda.is_current_stream_capturing()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                lo_r, iou_r, _ = self.right(src, self.key_pe, text, self.cfg.grid)
            lo_l, iou_l, tax = self.left(src, self.key_pe, text, self.cfg.grid, taps)
            cur.wait_stream(side)
            if not capturing:   # allocator bookkeeping for tensors that crossed streams (graph pools need none)
                for t in (src, text):
                    t.record_stream(side)
                for t in (lo_r, iou_r):
                    t.record_stream(cur)
            return lo_l, lo_r, tax, iou_l, iou_r
        lo_l, iou_l, tax = self.left(src, self.key_pe, text, self.cfg.grid, taps)
        lo_r, iou_r, _ = self.right(src, self.key_pe, text, self.cfg.grid)
        return lo_l, lo_r, tax, iou_l, iou_r

    def postprocess(self, low_res, input_size, original_size):
        """Sam.postprocess_masks (sam.py:177-188): x4 bilinear to img_size, crop, bilinear to original size."""
        S = self.cfg.img_size
        m = ops.resize_bilinear(low_res, low_res.shape[-2:], (S, S))
        if tuple(input_size) == (S, S) and tuple(original_size) == (S, S):
            return m  # second interpolate is the identity (scale 1, lambda 0)
        return ops.resize_bilinear(m, input_size, original_size)
