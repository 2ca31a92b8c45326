"""4-bit NF4 language-model weights: the reference's `load_in_4bit=True` (2Haff/inference.py:133-146, chat.py the same) on the fp16
mode's kernels.

The reference loads `LISAForCausalLM.from_pretrained(..., torch_dtype=torch.half, quantization_config=BitsAndBytesConfig(
load_in_4bit=True, bnb_4bit_compute_dtype=torch.float16, bnb_4bit_use_double_quant=True, bnb_4bit_quant_type="nf4",
llm_int8_skip_modules=["visual_model"]))`. bitsandbytes is not a dependency of this project; what follows RESTATES its format
(README, "What stays unpinned"):

Which Linears become NF4 (`nf4_linear`): every nn.Linear that exists when from_pretrained runs and whose name does not contain
"visual_model" — the Llama q/k/v/o/gate/up/down_proj, model.mm_projector (llava_arch.py:35), both text_hidden_fcs Linears
(LISA.py:71-77) and lm_head (transformers 4.31 uses llm_int8_skip_modules INSTEAD of its default keep-list, so lm_head is
converted too; restated, 4.31 is not installed here: `nf4_lm_head=False` keeps it fp16). SAM, the CLIP tower (loaded later by
initialize_vision_modules), embed_tokens, the norms and the biases stay fp16.

NF4 quantisation of one weight tensor W (fp16, after the fp16 mode's conversion check):
  * W flattened row-major into blocks of 64 (every Linear here has K % 64 == 0, so a block never crosses a row);
  * absmax = fp32 max |w| of the block;
  * code = index of the NF4 value nearest to w * (1/absmax) (fp32 reciprocal, correctly rounded, then one fp32 multiply);
    the decision thresholds are the fp32 midpoints of neighbouring NF4 values and a value exactly on one takes the LOWER code;
    an all-zero block (absmax 0) gets code 7 (the value 0) everywhere. Either way such weights dequantise to 0;
  * two codes per byte, the first element in the high nibble.
Double quantisation (bnb_4bit_use_double_quant=True):
  * offset = mean of the tensor's absmax values (here: summed in double, in a fixed order, rounded once to fp32);
  * absmax - offset (fp32) is quantised in blocks of 256 consecutive values with the signed 8-bit dynamic map
    (`dynamic_map()`, bitsandbytes' create_dynamic_map(signed=True) restated from its construction): absmax2 = fp32 max |.| of
    the block, code = nearest map value to (absmax - offset) * (1/absmax2) (same midpoint rule; absmax2 == 0: the code of 0);
  * dequantised absmax = map[code] * absmax2 + offset: an fp32 multiply, then an fp32 add (not fused).
What enters a product: f16_rn(NF4[code] * absmax_dq), one fp32 multiply and one rounding — what bitsandbytes' dequantize_4bit
returns for an fp16 compute dtype — then the fp16 mode's f16 MFMA product with fp32 accumulation. (For one-row inputs bitsandbytes
runs gemv_4bit instead, whose summation order differs: within fp16 noise of the same values.)

Storage here is row-local (csrc/gemm_nf4.hip): packed uint8 [N][K/2] and the DEQUANTISED absmax fp32 [N][K/64], so the q|k|v
concatenation, the SwiGLU interleave and the RoPE row permutation are row reorders of stored NF4 rows; each source tensor is still
quantised on its own, as the reference quantises each Linear. 4.5 bits per weight (bitsandbytes keeps the 8-bit absmax codes: 4.13).
"""
import re

import torch

from . import ops

# bitsandbytes' NF4 code values
NF4_VALUES = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
              -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
              0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)


def nf4_table():
    return torch.tensor(NF4_VALUES, dtype=torch.float32)


def dynamic_map():
    """The signed 8-bit dynamic map (256 fp32 values, sorted): for decade i = 0..6, the 2^i means of neighbouring points of
    linspace(0.1, 1, 2^i + 1) (float32) times 10^(i - 6), with both signs; then 0 and +1 (the construction has no -1)."""
    data = []
    for i in range(7):
        b = torch.linspace(0.1, 1, 2 ** i + 1)
        means = (b[:-1] + b[1:]) / 2.0
        data += ((10 ** (i - 6)) * means).tolist()
        data += (-(10 ** (i - 6)) * means).tolist()
    data += [0.0, 1.0]
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


_LLAMA_PROJ = re.compile(r"^model\.layers\.\d+\.(self_attn\.(q|k|v|o)_proj|mlp\.(gate|up|down)_proj)\.weight$")


def nf4_linear(name, lm_head=True):
    """True for the weight of an nn.Linear the reference's 4-bit load converts (module selection above)."""
    if "visual_model" in name or not name.endswith(".weight"):
        return False
    if _LLAMA_PROJ.match(name):
        return True
    if name in ("model.mm_projector.weight", "model.text_hidden_fcs.0.0.weight", "model.text_hidden_fcs.0.2.weight"):
        return True
    return lm_head and name == "lm_head.weight"


class Nf4Weight:
    """An NF4 weight on the device: packed uint8 [N, K/2], dequantised absmax f32 [N, K/64]."""

    def __init__(self, packed, absmax):
        self.packed, self.absmax = packed, absmax
        self.shape = (packed.shape[0], packed.shape[1] * 2)
        self.lora = None   # Nf4Lora: unmerged adapters served on top of the codes (lora_pack)

    @property
    def nbytes(self):
        return self.packed.numel() + self.absmax.numel() * 4

    def dequant(self, row_map=None, out=None):
        if self.lora is not None:
            return ops.nf4_dequant_lora(self.packed, self.absmax, self.lora, row_map=row_map, out=out)
        return ops.nf4_dequant(self.packed, self.absmax, row_map=row_map, out=out)

    def dequant_t(self, row_map=None, out=None):
        """The transpose of dequant() as f16 [K, roundup(N, 8)] (pad columns zero): W^T of a dX product, written from the codes."""
        return ops.nf4_dequant_t(self.packed, self.absmax, row_map=row_map, out=out)


def quantize(parts, device, double_quant=True):
    """One Nf4Weight from source weights quantised EACH ON ITS OWN (as the reference quantises each Linear): parts = [(w, rows)],
    w [n_i, K] (any float dtype, any device), rows = int tensor [n_i] of destination rows, or None (the rows stacked in order)."""
    K = parts[0][0].shape[1]
    R = sum(w.shape[0] for w, _ in parts)
    packed = torch.empty((R, K // 2), dtype=torch.uint8, device=device)
    absmax = torch.empty((R, K // 64), dtype=torch.float32, device=device)
    r0 = 0
    for w, rows in parts:
        n = w.shape[0]
        if rows is None:
            rows = torch.arange(r0, r0 + n)
        rmap = rows.to(device=device, dtype=torch.int32)
        w16 = w.to(device=device, dtype=torch.float16).contiguous()
        ops.nf4_quantize(w16, double_quant=double_quant, row_map=rmap, packed=packed, absmax=absmax)
        del w16
        r0 += n
    return Nf4Weight(packed, absmax)


# ---------------------------------------------------------------------------------------------------------------------------------
# Unmerged LoRA adapters on NF4 weights: serving what `train_ds.py --load_in_4bit` (QLoRA) fitted against the codes
# ---------------------------------------------------------------------------------------------------------------------------------
# The trainer optimised y = x deq(Q(W))^T + s (x A^T) B^T. Merging s B A into the 16-bit W and quantising again serves another
# function (the second quantisation's error exceeds a small adapter's whole effect), so the adapters stay
# beside the codes. Per fused weight: A_cat f16 [8 nseg, K] (8 rank rows per row segment: q | k | v, gate | up, or the one of o /
# down; rank < 8 zero-padded, an unadapted segment zero) and B f16 [N, 8] in the STORED row order (the quantiser's row maps).
LORA_MAX_RANK = 8   # the fused training nodes' limit (autograd.py), and the 8 k-slots of a segment in the decode kernel's MFMA
LORA_PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_LORA_MODULE = re.compile(r"^model\.layers\.(\d+)\.(self_attn\.(q|k|v|o)_proj|mlp\.(gate|up|down)_proj)$")


class Nf4Lora:
    """The adapters of one fused NF4 weight on the device (layout above); scale = lora_alpha / r."""

    def __init__(self, a_cat, b, nseg, seg_rows, scale):
        self.a_cat, self.b, self.nseg, self.seg_rows, self.scale = a_cat, b, int(nseg), int(seg_rows), float(scale)

    @property
    def nbytes(self):
        return (self.a_cat.numel() + self.b.numel()) * 2


def lora_pairs(lora_state, cfg):
    """{module: (A [r, in], B [out, r])} of a LisaTrainable.state_dict()'s `.lora_A` / `.lora_B` keys, checked on the host against the
    Llama geometry of cfg: a module outside the seven projections of an existing layer, a missing half of a pair, rank > 8, ranks
    that differ between modules (one scale alpha / r serves a fused weight) and shapes that do not fit raise ValueError naming the
    module. Returns (pairs, r) (r None without adapters)."""
    H, F = cfg.llm.hidden, cfg.llm.ffn
    dims = {"q_proj": (H, H), "k_proj": (H, H), "v_proj": (H, H), "o_proj": (H, H), "gate_proj": (H, F), "up_proj": (H, F),
            "down_proj": (F, H)}   # (in_features, out_features)
    if H % 16:
        raise ValueError(f"lora_state: the q | k | v row segments need hidden % 16 == 0 (hidden = {H})")
    pairs, rank = {}, None
    mods = sorted({k.rsplit(".", 1)[0] for k in lora_state if k.endswith(".lora_A") or k.endswith(".lora_B")})
    for mod in mods:
        m = _LORA_MODULE.match(mod)
        if not m or int(m.group(1)) >= cfg.llm.layers:
            raise ValueError(f"lora_state: {mod} is not one of the Llama projections ({', '.join(LORA_PROJ)} of layers 0.."
                             f"{cfg.llm.layers - 1}); adapters are served on those only")
        if mod + ".lora_A" not in lora_state or mod + ".lora_B" not in lora_state:
            raise ValueError(f"lora_state: {mod} has only one of .lora_A / .lora_B")
        a, b = lora_state[mod + ".lora_A"], lora_state[mod + ".lora_B"]
        fin, fout = dims[mod.rsplit(".", 1)[1]]
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != fin or b.shape[0] != fout or b.shape[1] != a.shape[0] or a.shape[0] < 1:
            raise ValueError(f"lora_state: {mod}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit a [{fout}, {fin}] "
                             f"weight (expected [r, {fin}] and [{fout}, r])")
        r = a.shape[0]
        if r > LORA_MAX_RANK:
            raise ValueError(f"lora_state: {mod} has rank {r}; adapters are served up to rank {LORA_MAX_RANK}")
        if rank is not None and r != rank:
            raise ValueError(f"lora_state: {mod} has rank {r}, other modules {rank}; one lora_alpha / r serves every adapter")
        rank = r
        pairs[mod] = (a, b)
    return pairs, rank


def lora_pack(parts, K, seg_rows, scale, device):
    """Nf4Lora of a fused weight from its source weights' adapters, in quantize()'s order and with its row maps: parts =
    [(pair or None, n_i, rows or None)], pair = (A [r, K], B [n_i, r]). None when no part is adapted."""
    if all(pair is None for pair, _, _ in parts):
        return None
    nseg = len(parts)
    R = sum(n for _, n, _ in parts)
    a_cat = torch.zeros((8 * nseg, K), dtype=torch.float16)
    b_all = torch.zeros((R, 8), dtype=torch.float16)
    r0 = 0
    for i, (pair, n, rows) in enumerate(parts):
        if rows is None:
            rows = torch.arange(r0, r0 + n)
        if pair is not None:
            a, b = pair
            r = a.shape[0]
            a_cat[8 * i:8 * i + r] = a.detach().to("cpu", torch.float16)
            b_all[rows, :r] = b.detach().to("cpu", torch.float16)
        r0 += n
    return Nf4Lora(a_cat.to(device).contiguous(), b_all.to(device).contiguous(), nseg, seg_rows, scale)


def swiglu_rows(F):
    """Destination rows of gate and up in the [gate x16 | up x16] interleave of LlamaHip."""
    r = torch.arange(F)
    base = (r // 16) * 32 + r % 16
    return base, base + 16


def rope_row_map(N, device):
    """Output row map of the dequantisation that yields ops.rope_permute_rows(w): stored row idx[r] -> row r."""
    j = torch.arange(256)
    wn, t, i = j // 64, (j // 16) % 4, j % 16
    logical = (wn // 2) * 128 + (t // 2) * 64 + (wn % 2) * 32 + (t % 2) * 16 + i
    idx = (torch.arange(0, N, 256)[:, None] + logical[None, :]).reshape(-1)
    inv = torch.empty_like(idx)
    inv[idx] = torch.arange(N)
    return inv.to(device=device, dtype=torch.int32)


def round_trip(w, device, double_quant=True):
    """f16 dequant(quantize(w)): the values of an NF4 Linear whose product keeps its 16/32-bit path (mm_projector,
    text_hidden_fcs)."""
    return quantize([(w, None)], device, double_quant).dequant()


# ---------------------------------------------------------------------------------------------------------------------------------
# LLM.int8: the reference's `load_in_8bit=True` (2Haff/inference.py:147-156; chat.py / app.py the same)
# ---------------------------------------------------------------------------------------------------------------------------------
# LLM.int8 language-model weights (bitsandbytes 0.41.1 `BitsAndBytesConfig(load_in_8bit=True, llm_int8_skip_modules=
# ["visual_model"])` under transformers 4.31.0: llm_int8_threshold 6.0, llm_int8_has_fp16_weight False), RESTATED — bitsandbytes is not
# a dependency, and the steps below are what this project computes (README, "What stays unpinned": the constant C and whether the row
# absmax skips outlier elements or whole columns).
#
# Module selection: that of the 4-bit load (`nf4_linear`; `int8_lm_head=False` keeps lm_head fp16).
#
# Weights (Int8Params.cuda -> double_quant(W), threshold 0), per output row n:
#   SCB[n] = fp32 max |W[n, :]|;  CB[n, k] = rint(f32(W[n, k]) * (127.0f / SCB[n]))  (one fp32 division per row, then one fp32 multiply
#   per weight, rint = round half to even); SCB 0: every code 0.
# Every call of a converted Linear (MatMul8bitLt.forward) on fp16 rows A [M, K], threshold t:
#   1. outlier elements: |a| >= t (t = 0: none);
#   2. SCA[m] = fp32 max |a| over row m's NON-OUTLIER elements (0 if there are none);
#   3. CA[m, k] = rint(a * (127.0f / SCA[m])), 0 for an outlier element; SCA[m] = 0: every code 0 (bitsandbytes would compute 0 * inf);
#   4. idx = the sorted columns holding an outlier in ANY row of the call; CA[:, idx] = 0 in every row;
#   5. subA = A[:, idx] (fp16), subB = f16((f32(CB[:, idx]) * SCB[:, None]) / 127.0f) (a division, not a reciprocal multiply);
#   6. Y = f16(f32(CA . CB^T) * C * SCA[m] * SCB[n] + bias[n]), left to right, each operation rounded to fp32 (no contraction);
#      C = 6.200012e-05f; the int32 accumulation is exact (|acc| <= 127^2 * 11008 < 2^31);
#   7. if idx is not empty: Y = f16(f32(Y) + f32(f16(subA . subB^T))), the outlier product a fixed-order fp32 sum over ascending columns
#      (f16 x f16 is exact in fp32, so fma and multiply-then-add agree).
# Whose rows form "the call": the reference generates with use_cache=False (LISA.py:115), one frame per call, recomputing the whole
# prefix for every token. A SEGMENT here is one frame's valid rows; idx is per segment, never over a batch, never over padding rows.
# KV-cached decoding keeps per-(frame, Linear input) STICKY column masks — the prefill sets them from the frame's rows, every decode step
# ORs its row's outliers in before quantising — so the newest row is quantised exactly as the reference's last row. Deviation left:
# when a decode step adds a column the reference would requantise the earlier rows too; their cached K / V keep the old values.


def int8_quantize_weight_cpu(w):
    """(CB int8 [N, K], SCB f32 [N]) of a weight (any float dtype; rounded to fp16 first, as the reference loads it)."""
    w = w.to(torch.float16).float()
    scb = w.abs().amax(1)
    s = torch.where(scb > 0, torch.tensor(127.0, dtype=torch.float32) / scb, torch.zeros_like(scb))
    return torch.round(w * s[:, None]).to(torch.int8), scb


def int8_quantize_rows_cpu(a, threshold, seg_rows=None, valid=None, masks=None):
    """Steps 1-4 on fp16 rows a [M, K]: -> (CA int8 [M, K], SCA f32 [M], cols bool [S, K]). Segments of seg_rows rows (None: one),
    valid[s] of them counting (None: all); masks (bool [S, K]) are ORed into in place (the sticky masks) when given."""
    a = a.to(torch.float16).float()
    M, K = a.shape
    seg_rows = M if seg_rows is None else seg_rows
    S = (M + seg_rows - 1) // seg_rows
    out = (a.abs() >= threshold) if threshold > 0 else torch.zeros_like(a, dtype=torch.bool)
    sca = torch.where(out, torch.zeros_like(a), a.abs()).amax(1)
    seg = torch.arange(M) // seg_rows
    ok = torch.ones(M, dtype=torch.bool) if valid is None else (torch.arange(M) - seg * seg_rows) < torch.as_tensor(valid)[seg]
    cols = torch.zeros((S, K), dtype=torch.bool) if masks is None else masks
    for s in range(S):
        rows = (seg == s) & ok
        cols[s] |= out[rows].any(0)
    sc = torch.where(sca > 0, torch.tensor(127.0, dtype=torch.float32) / sca, torch.zeros_like(sca))
    ca = torch.round(a * sc[:, None])
    ca = torch.where(out | cols[seg], torch.zeros_like(ca), ca)
    return ca.to(torch.int8), sca, cols


INT8_C = 6.200012e-05


def int8_linear_cpu(a, cb, scb, ca, sca, cols, seg_rows=None, bias=None):
    """Steps 5-7: the f16 Y [M, N] of a converted Linear from the quantised rows (int8_quantize_rows_cpu) and weights."""
    a = a.to(torch.float16).float()
    M = a.shape[0]
    seg_rows = M if seg_rows is None else seg_rows
    acc = (ca.long() @ cb.long().t()).float()
    c = torch.tensor(INT8_C, dtype=torch.float32)
    t = acc * c
    t = t * sca[:, None]
    t = t * scb[None, :]
    if bias is not None:
        t = t + bias.float()[None, :]
    y = t.half().float()
    seg = torch.arange(M) // seg_rows
    for s in range(cols.shape[0]):
        idx = cols[s].nonzero().flatten()
        rows = (seg == s).nonzero().flatten()
        if idx.numel() == 0 or rows.numel() == 0:
            continue
        sub_b = ((cb[:, idx].float() * scb[:, None]) / 127.0).half().float()      # [N, n]
        sub_a = a[rows][:, idx]                                                   # [r, n]
        o = torch.zeros((rows.numel(), cb.shape[0]), dtype=torch.float32)
        for j in range(idx.numel()):                                              # fixed order: ascending columns
            o = o + sub_a[:, j:j + 1] * sub_b[None, :, j]
        y[rows] = (y[rows] + o.half().float()).half().float()
    return y.half()


class Int8Weight:
    """An LLM.int8 weight on the device: CB int8 [N, K], SCB f32 [N] (no fp16 copy is kept)."""

    def __init__(self, cb, scb):
        self.cb, self.scb = cb, scb
        self.shape = tuple(cb.shape)

    @property
    def nbytes(self):
        return self.cb.numel() + self.scb.numel() * 4


def quantize_int8(parts, device):
    """One Int8Weight from source weights parts = [(w, rows)] (rows: int tensor of destination rows, or None: stacked in order). Row
    quantisation is row-local, so the q|k|v concatenation and the SwiGLU interleave are row reorders of CB / SCB."""
    K = parts[0][0].shape[1]
    R = sum(w.shape[0] for w, _ in parts)
    cb = torch.empty((R, K), dtype=torch.int8, device=device)
    scb = torch.empty((R,), dtype=torch.float32, device=device)
    r0 = 0
    for w, rows in parts:
        n = w.shape[0]
        if rows is None:
            rows = torch.arange(r0, r0 + n)
        w16 = w.to(device=device, dtype=torch.float16).contiguous()
        ops.int8_quantize_weight(w16, row_map=rows.to(device=device, dtype=torch.int32), cb=cb, scb=scb)
        del w16
        r0 += n
    return Int8Weight(cb, scb)


int8_linear = nf4_linear   # the same module selection
