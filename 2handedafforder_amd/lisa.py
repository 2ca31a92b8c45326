"""LISAForCausalLM for MI355X — the drop-in boundary of the 2Haff hot path.

`LisaMI355.evaluate(images_clip, images, input_ids, resize_list, original_size_list, max_new_tokens=32,
tokenizer=None)` has the signature and return tuple of the reference's `LISAForCausalLM.evaluate`
(2Haff/model/LISA.py:432-534): (output_ids, pred_masks_left, pred_masks_right, taxonomies); `predict` is
the alias BASELINE.json's north_star names. All numerics run in the HIP kernels of csrc/ through the C-ABI;
torch only owns HBM allocations, views and the stream.

Differences from the reference that do NOT change results:
  * KV-cached greedy decode (reference: use_cache=False, LISA.py:115, recomputes CLIP + prefix every token);
  * text_hidden_fcs runs only on the [SEG]-selected rows (reference: on all T positions, then masks, :467-473);
  * frames / prompts are batched through the SAM encoder and decoders (reference: python loops, :157-168,494-532).
Extension for synthetic benchmarking: `forced_answer` overrides the appended tokens (argmax still computed).
"""
import contextlib
import json
import os

import torch

from . import ops, overlap, prompt_groups
from .llava import ClipTowerHip, LlamaHip, _f32
from .sam import SamEncoderHip, SamPromptDecoderHip

IMAGE_TOKEN_INDEX = -200
N_IMG_PAD = 255  # LISA.py:461


def _check_fp16_weights(sd, device):
    """The fp16 mode's weight conversion (the reference's `model.half()`), checked tensor by tensor on the device: a value that turns
    non-finite (|w| > 65504) raises ValueError naming the tensor. Returns how many nonzero weights flushed to zero (|w| below half the
    smallest fp16 subnormal) and warns when there are any."""
    flushed = 0
    for name, t in sd.items():
        if not torch.is_floating_point(t):
            continue
        src = t.to(device)
        h = src.to(torch.float16)
        bad = int((~torch.isfinite(h) & torch.isfinite(src)).sum())
        if bad:
            raise ValueError(f"fp16 mode: {bad} weights of {name} do not fit fp16 (|w| > 65504; max |w| = {src.abs().max().item():.6g})")
        flushed += int(((h == 0) & (src != 0)).sum())
        del src, h
    if flushed:
        import warnings
        warnings.warn(f"fp16 mode: {flushed} nonzero weights flushed to zero in the fp16 conversion")
    return flushed


class LisaMI355:
    def __init__(self, cfg, state_dict, dtype=torch.bfloat16, device="cuda:0", sam_chunk=8, fp32_tail=True, fp32_stream=False,
                 neck_f32=False, load_in_4bit=False, bnb_4bit_use_double_quant=True, bnb_4bit_quant_type="nf4", nf4_lm_head=True,
                 load_in_8bit=False, llm_int8_threshold=6.0, llm_int8_has_fp16_weight=False, int8_lm_head=True, lora_state=None,
                 lora_alpha=16):
        # load_in_4bit: the reference's bitsandbytes 4-bit load (inference.py:133-146): the fp16 mode with the Llama projections,
        # mm_projector, text_hidden_fcs and (nf4_lm_head) lm_head quantised to NF4 (quant.py). Refused combinations are ValueErrors
        if load_in_4bit:
            if dtype != torch.float16:
                raise ValueError("load_in_4bit: the reference's 4-bit mode computes in float16 (bnb_4bit_compute_dtype=torch.float16); "
                                 f"pass dtype=torch.float16, not {dtype}")
            if bnb_4bit_quant_type != "nf4":
                raise ValueError(f"load_in_4bit: bnb_4bit_quant_type={bnb_4bit_quant_type!r} is not supported (only 'nf4')")
        # load_in_8bit: the reference's bitsandbytes 8-bit load (inference.py:147-156): the fp16 mode with the same Linears as LLM.int8
        # (quant.py) on the int8 matrix cores
        if load_in_8bit:
            if load_in_4bit:
                raise ValueError("load_in_4bit and load_in_8bit are exclusive (the reference's CLIs take one or the other)")
            if dtype != torch.float16:
                raise ValueError("load_in_8bit: the reference's 8-bit mode computes in float16 (torch_dtype=torch.half); "
                                 f"pass dtype=torch.float16, not {dtype}")
            if llm_int8_has_fp16_weight:
                raise ValueError("load_in_8bit: llm_int8_has_fp16_weight=True (the 8-bit training layout) is not supported")
            if not llm_int8_threshold >= 0:
                raise ValueError(f"load_in_8bit: llm_int8_threshold must be >= 0 (got {llm_int8_threshold})")
        # lora_state (load_in_4bit only): LisaTrainable.state_dict() of an NF4 fine-tune (train_ds.py --load_in_4bit: latest.pt["params"]).
        # Its .lora_A / .lora_B pairs are served UNMERGED on the NF4 codes, y = x deq(W)^T + (lora_alpha / r) (x A^T) B^T: the function
        # the trainer optimised (merging and quantising again is not: DESIGN.md section 8). Its other tensors (embed_tokens, lm_head,
        # text_hidden_fcs, both mask decoders) replace the same-named entries of state_dict, and the quantised set becomes the
        # trainer's (train_model.nf4_frozen_linear): lm_head and text_hidden_fcs stay as trained, mm_projector stays NF4
        lora_pairs, lora_rank = {}, None
        if lora_state is not None:
            if not load_in_4bit:
                raise ValueError("lora_state: unmerged adapters are served on the NF4 base only (load_in_4bit=True); 16-bit bases are "
                                 "served merged (merge_lora.py)")
            from . import quant
            lora_pairs, lora_rank = quant.lora_pairs(lora_state, cfg)
            state_dict = dict(state_dict)
            state_dict.update({k: v for k, v in lora_state.items() if not (k.endswith(".lora_A") or k.endswith(".lora_B"))})
            nf4_lm_head = False
        if not torch.cuda.is_available():
            raise RuntimeError("LisaMI355 needs an MI355X (HIP device); there is no CPU fallback for the hot path")
        from .lib import load_library
        load_library()  # fail loudly if the HIP library is absent
        if dtype == torch.float16 and (fp32_stream or neck_f32 or not fp32_tail):
            # the fused fp32 stream is a bf16 epilogue, the fp16 mode runs the ViT-H neck in f32 by contract, and the decoder tail's
            # kernels (sam_decoder.hip) have no f16 rows: the fp16 mode's tail is fp32
            raise ValueError("LisaMI355(dtype=torch.float16): fp32_stream, neck_f32 and fp32_tail=False are bf16-mode options "
                             "(the fp16 neck and decoder tail are always f32)")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.seg_token_idx = cfg.seg_token_idx
        self.sam_chunk = sam_chunk
        self._sam_stream = torch.cuda.Stream(device=self.device)
        # How the encoder's stream shares the CUs with the decode steps (overlap.py): "auto" = the work-model plan per
        # evaluate() call, None = every launch on all CUs, or an explicit list of workgroup caps per encoder chunk;
        # sam_waits_for_prefill "auto" | True | False (late mode: the encoder starts behind the prefill on the GPU too).
        self.sam_chunk_caps = "auto"
        self.sam_waits_for_prefill = "auto"
        self.calibrate_overlap = True         # False: the plan uses overlap.NOMINAL (round 5's fitted constants) whatever the device
        self.last_rates = None
        self.expected_new_tokens = 8          # what the plan assumes a reply takes ("Sure, ... [SEG] ." templates) when max_new_tokens is larger
        self._plan = (None, False, None)      # (caps, wait, chunk) of the evaluate() call in flight (no caps outside one)
        self.last_plan = (None, False, None)  # ... of the last evaluate() call (what bench.py reports)
        self.last_decode_chain = False
        # The SAM encoder runs on its own HIP stream beside the language model and joins before the mask decoders
        # (+4-5 % frames/s); False serialises everything on the caller's stream (per-kernel measurements). Results are
        # bit-identical either way (tests/test_fullsize_gpu.py; the history of that check: DESIGN.md section 10a).
        self.overlap_streams = True
        self.sam_beside_decode = None   # None: by batch size (<= 4 frames: encoder enqueued behind the prefill); True / False force
        # KV-cached decode steps are launch-bound at small batch (32 layers x 9 launches per token): each step is
        # captured once per (batch, position) into a hipGraph and replayed. The KV cache is persistent per
        # (batch, capacity) so the captured pointers stay valid across evaluate() calls.
        self.decode_graphs = True
        # Decode steps of <= 8 rows as ONE chained launch per step (LlamaHip.decode_chain, csrc/decode_chain.hip). "auto": below
        # overlap.MIN_FRAMES (4) frames per call (round 6, same box: decode step 3.25 -> 3.11 ms at one row, one frame 41.3 -> 40.6 ms,
        # three frames 57.8 -> 56.7). From 4 frames on the plan caps the encoder to 128..192 CUs beside the decode steps, and there a
        # chained step's 80 000 workgroups keep refilling every slot of every CU while the encoder's one-per-CU launches wait — 4 / 8
        # frames lose 20..25 % — so the five short launches per layer stay. The choice depends on the batch alone, not on the schedule
        # (streams, caps): every schedule of a batch gives the same bits. True: chained at any batch <= 8 (A/B); False: never.
        # generate() called directly follows LlamaHip.decode_chain.
        self.decode_chain = "auto"
        # evaluate(): the last Llama layer of the prefill runs o_proj / MLP / final norm on the rows that are read only (LlamaHip.forward,
        # keep_rows; round 6). False: every row (A/B; generate() called directly always returns every row)
        self.prune_last_layer = True
        self._ingest = None
        self._graphs = {}
        # one memory pool shared by every captured step. Replays never overlap: every graph is replayed on the caller's stream,
        # one after another — the split-K workspaces baked into them (ops._workspace) may be the same buffer
        self._graph_pool = None
        self._caches = {}
        self._prefix_caches = {}
        # evaluate(offset=): what the last call did — frames, rows, shared_prefix_ids (ids of the prompt prefix prefilled once per frame),
        # prefix_positions (its cache positions), shared (that path was taken), encoder_frames (frames the encoders ran over)
        self.last_group_plan = None
        # True: the mask decoders run once per [SEG] row (the batch-1 launch sequence, replayed) instead of once over all rows. The fp32
        # products of the tail pick their kernel by row count (csrc/gemm_f32.hip), so a batched tail's bits depend on how many rows share
        # the call; per row they do not — robot_demo.py --multi_prompt wants an action's files not to depend on the other actions.
        # Costs one tail per row: off by default (throughput).
        self.tail_per_row = False
        sd, dev = state_dict, self.device
        self.fp16_flushed_weights = _check_fp16_weights(sd, dev) if dtype == torch.float16 else 0
        assert cfg.clip.n_patches == N_IMG_PAD + 1, "the reference hard-codes 256 image tokens (LISA.py:461)"
        # fp32 decoder tail (throughput mode): image embeddings leave the neck in fp32 and text_hidden_fcs, the prompt
        # encoder, both two-way mask decoders, the hypernetwork / IoU / taxonomy MLPs and the upscaler run on the
        # f32-input matrix cores (csrc/gemm_f32.hip) — 7 GFLOP of the 10 TFLOP per frame (hard part 3).
        # The ViT-H / CLIP / Llama stacks stay bf16 MFMA. False = the all-bf16 path of round 1.
        self.fp32_tail = fp32_tail and dtype in (torch.bfloat16, torch.float16)
        tail = torch.float32 if self.fp32_tail else dtype
        self.tail_dtype = tail
        self.sam_encoder = SamEncoderHip(sd, cfg.sam, dtype, dev)
        self.sam_encoder.emb_f32 = self.fp32_tail
        self.sam_decoder = SamPromptDecoderHip(sd, cfg.sam, tail, dev)
        self.clip = ClipTowerHip(sd, cfg.clip, dtype, dev)
        self.load_in_4bit = bool(load_in_4bit)
        self.load_in_8bit = bool(load_in_8bit)
        self.llm_int8_threshold = float(llm_int8_threshold)
        self.llm = LlamaHip(sd, cfg.llm, dtype, dev, nf4=self.load_in_4bit, nf4_double_quant=bnb_4bit_use_double_quant,
                            nf4_lm_head=nf4_lm_head, int8=self.load_in_8bit, int8_threshold=self.llm_int8_threshold,
                            int8_lm_head=int8_lm_head, lora=lora_pairs, lora_scale=(lora_alpha / lora_rank) if lora_rank else 0.0)
        # fp32 residual streams in the bf16 mode: True / "sam" / "llm" — the ViT-H and / or Llama hidden-state
        # stream kept in fp32 between the bf16 MFMA products (2.8x closer to the reference on the image embedding at depth 32)
        self.sam_encoder.fp32_stream = fp32_stream in (True, "sam", "both")
        self.llm.fp32_stream = fp32_stream in (True, "llm", "both")
        self.sam_encoder.neck_f32 = (bool(neck_f32) and dtype == torch.bfloat16) or dtype == torch.float16  # the ViT-H neck on the f32-input MFMA path (sam.py)
        def lin_w(name, dt):
            # 4-bit mode: mm_projector and text_hidden_fcs are NF4 Linears in the reference; their values are quantised and
            # dequantised once here and their products keep the 16 / 32-bit paths (their bytes are not what a frame waits for)
            if self.load_in_4bit and (lora_state is None or "text_hidden_fcs" not in name):
                from . import quant
                return quant.round_trip(sd[name], dev, bnb_4bit_use_double_quant).to(dt).contiguous()
            if self.load_in_8bit:
                # 8-bit mode: int8 products (ops.linear_int8), one segment per frame's rows (encode_images, seg_embeddings)
                from . import quant
                return quant.quantize_int8([(sd[name], None)], dev)
            return sd[name].to(dev, dt).contiguous()
        self.w_proj = lin_w("model.mm_projector.weight", dtype)
        self.b_proj = _f32(sd["model.mm_projector.bias"], dev)
        self.fc0 = (lin_w("model.text_hidden_fcs.0.0.weight", tail), _f32(sd["model.text_hidden_fcs.0.0.bias"], dev))
        self.fc2 = (lin_w("model.text_hidden_fcs.0.2.weight", tail), _f32(sd["model.text_hidden_fcs.0.2.bias"], dev))

    def llm_weight_bytes(self):
        """Device bytes of the Llama projections and lm_head (the weights a decode step streams)."""
        return self.llm.weight_bytes()

    # ---- a4/a5: CLIP tower + projector -------------------------------------------------------------------
    def encode_images(self, images_clip):
        B = images_clip.shape[0]
        images_clip = images_clip.to(self.device)

        def fn(x):
            if self.load_in_8bit:
                # the projector's call in the reference is one frame's 256 patch rows: one segment each (cls rows dropped first)
                n = self.cfg.clip.n_patches
                h = self.clip.hidden(x)
                rows = h.view(B, n + 1, -1)[:, 1:].reshape(B * n, -1)
                q = ops.int8_quantize_act(rows, self.llm_int8_threshold, n)
                return (ops.linear_int8(q, self.w_proj.cb, self.w_proj.scb, bias=self.b_proj).view(B, n, -1),)
            return (self.clip.project(self.clip.hidden(x), B, self.w_proj, self.b_proj),)
        if not self.decode_graphs or B > 4:
            return fn(images_clip)[0]
        return self._replay(("clip", B, images_clip.dtype, tuple(images_clip.shape[1:])), fn, [images_clip.contiguous()])[0]

    # ---- a6-a8: splice + greedy generate -----------------------------------------------------------------
    @torch.no_grad()
    def generate(self, images_clip, input_ids, max_new_tokens=32, forced_answer=None, attention_mask=None, after_prefill=None,
                 needed_hidden_only=False, frame_of=None):
        """Greedy KV-cached decode (LISA.py:443-450). Rows may have different prompt lengths: input_ids is right-padded
        (utils/dataset.py:90-93) and attention_mask [B, L] (bool, True on real tokens; None = every row is full length)
        marks the real prefix of each row, as collate_fn builds it (:144-150). Row b's generated tokens are appended right
        after ITS last real token, so output_ids [B, L + N] is left-aligned per row (pad_token_id behind the end) and the
        hidden states [B, T + N - 1, H] line up with it position by position — the [SEG] rule of LISA.py:457-465 then
        applies per row unchanged. Equal to B independent batch-1 runs.
        frame_of (int32 [B] on the CPU, prompt_groups.check_offset; None = one frame per row): images_clip holds F frames and row b
        reads frame frame_of[b]. The CLIP tower and the projector run over the F frames; when every row starts with the same ids up to
        and past the <image> sentinel, that prefix is prefilled once per frame and its K / V are broadcast to the rows
        (ops.kv_prefix_broadcast); the rows' own ids are then prefilled behind it. `last_group_plan` says what was done."""
        cfg = self.cfg
        input_ids = input_ids.to(self.device)
        B, L = input_ids.shape
        is_img = input_ids == IMAGE_TOKEN_INDEX
        assert bool((is_img.sum(1) == 1).all()), "exactly one <image> sentinel per row (LISA.py:458 hack)"
        img_pos = is_img.int().argmax(1).to(torch.int32)
        if attention_mask is None:
            lens = torch.full((B,), L, dtype=torch.int64, device=self.device)
        else:
            am = attention_mask.to(self.device).bool()
            lens = am.sum(1)
            assert bool((am == (torch.arange(L, device=self.device)[None, :] < lens[:, None])).all()), "right padding only"
            assert bool((img_pos.long() < lens).all())
        img = self.encode_images(images_clip)
        n_img = img.shape[1]
        T = L + n_img - 1
        t_rows = lens + (n_img - 1)                      # real positions per row after the splice
        P = 0                                            # ids of the prefix that is prefilled once per frame (0: the plain prefill)
        if frame_of is not None:
            F = img.shape[0]
            # the 8-bit mode's sticky outlier masks are defined per frame over ALL of its prefill rows: splitting the prefill would
            # change them, so it prefills every row whole (as does a call whose rows share nothing, or one row per frame at most)
            if not self.load_in_8bit and int(torch.bincount(frame_of.long(), minlength=1).max()) >= 2:
                P = prompt_groups.shared_prefix_len(input_ids, lens, self.seg_token_idx)
            self.last_group_plan = {"frames": F, "rows": B, "shared_prefix_ids": P, "prefix_positions": prompt_groups.prefix_positions(P, n_img),
                                    "shared": P > 0, "encoder_frames": F}
            frame_of = frame_of.to(self.device)
            if P == 0:
                img = img.index_select(0, frame_of.long())
        cache = self._persistent_cache(B, T + max_new_tokens)
        st = cache["book"]
        p0 = P + n_img - 1 if P > 0 else 0               # cache positions filled by the broadcast: `prefill` below starts there
        if P > 0:
            # the F prefix rows (every row's first P ids are row 0's) through all layers into a cache of their own, no hidden state kept
            pre = self._prefix_cache(img.shape[0], p0)
            xp = ops.embed_splice(input_ids[:1, :P].clamp_min(IMAGE_TOKEN_INDEX).expand(img.shape[0], P).contiguous(),
                                  img_pos[:1].expand(img.shape[0]).contiguous(), self.llm.embed, img.contiguous())
            self.llm.forward(xp, pre, keep_rows=torch.empty((0,), dtype=torch.int64, device=self.device))
            for li in range(len(self.llm.layers)):
                ops.kv_prefix_broadcast(pre["k"][li], pre["v"][li], cache["k"][li], cache["v"][li], frame_of, p0)
            cache["len"] = p0
            # the rows' own ids: plain embedding rows (no sentinel behind the prefix), right-padded as before
            x = self.llm.embed.index_select(0, input_ids[:, P:].reshape(-1)).view(B, L - P, -1)
        else:
            # the sentinel slot itself is never dereferenced by the splice kernel
            x = ops.embed_splice(input_ids.clamp_min(IMAGE_TOKEN_INDEX).contiguous(), img_pos, self.llm.embed, img.contiguous())
        keep = None
        if needed_hidden_only and self.prune_last_layer and not self.load_in_8bit:
            # evaluate() reads two kinds of prefill rows only: each row's last real position (the first token's logits) and the
            # positions in front of a [SEG] that is part of the PROMPT (LISA.py:457-465 gathers the state that precedes the token);
            # the last Llama layer skips o_proj / MLP / norm for every other row (LlamaHip.forward, keep_rows)
            b_last = torch.arange(B, device=self.device) * T + (t_rows - 1)
            pb, pt = ((input_ids[:, 1:] == self.seg_token_idx) &
                      (torch.arange(1, L, device=self.device)[None, :] < lens[:, None])).nonzero(as_tuple=True)
            # id position j + 1 holds [SEG] -> seg_embeddings reads hidden row j + 255 (the reference's fixed 255-row shift, wherever
            # the <image> sentinel sits: LISA.py:459-463)
            keep = torch.unique(torch.cat([b_last, pb * T + pt + (n_img - 1)]))
            if p0:
                # the same rows counted in the [B, T - p0] tail: none of them lies in the shared part (shared_prefix_len, rules ii / iii)
                keep = (keep // T) * (T - p0) + (keep % T - p0)
        i8 = {"valid": t_rows.to(torch.int32)} if self.load_in_8bit else {}
        prefill = self.llm.forward(x, cache, keep_rows=keep, **i8)   # causal: a row's real positions never see its padding
        if after_prefill is not None:                    # work the caller wants enqueued (elsewhere) behind the prefill
            after_prefill()
        hidden, out_ids = st["hidden"], st["out_ids"]    # persistent [B, tmax, H] / [B, tmax]: the decode graph writes into them
        if p0:
            hidden[:, :p0].zero_()                       # never gathered: no [SEG] reads a hidden row of the shared part
        hidden[:, p0:T] = prefill
        hidden[:, T:].zero_()
        out_ids.fill_(cfg.pad_token_id)
        out_ids[:, :L] = torch.where(torch.arange(L, device=self.device)[None, :] < lens[:, None], input_ids,
                                     torch.full_like(input_ids, cfg.pad_token_id))
        if max_new_tokens <= 0:
            return out_ids[:, :L].clone(), hidden[:, :T - 1].clone()
        st["t_rows"].copy_(t_rows)
        st["lens"].copy_(lens)
        st["steps"].zero_()
        st["finished"].zero_()
        if forced_answer is not None:
            assert forced_answer.shape[0] == B and forced_answer.shape[1] >= max_new_tokens
            st["forced"][:, :max_new_tokens] = forced_answer[:, :max_new_tokens].to(self.device)
        st["use_forced"].fill_(0 if forced_answer is None else 1)
        rows = torch.arange(B, device=self.device)
        logits = self.llm.next_token_logits(prefill[rows, t_rows - (1 + p0)].contiguous())
        # token 0 (from the prefill logits), then one decode step per further token: embedding of the token just written ->
        # layers at each row's own position -> logits -> argmax -> bookkeeping of the next token, all device-side; the host
        # only reads the rows' finished flags between steps (generate()'s stopping rule)
        ops.decode_book(ops.argmax_rows(logits), st, None, cfg.pad_token_id, cfg.eos_token_id)
        n_done = 1
        while n_done < max_new_tokens and not bool(st["finished"].all()):
            self._decode_book_step(cache)
            n_done += 1
        ch = cache.get("chain")
        if ch is not None and n_done > 1 and not ops.decode_chain_status(ch["sync"], len(self.llm.layers)):
            # a bounded wait of the chained decode launch ran out (csrc/decode_chain.hip): the tokens above are garbage — fail loudly
            ch["sync"].zero_()
            raise RuntimeError("chained decode launch: a stage's arrival counter never filled (sticky error word set); "
                               "set LlamaHip.decode_chain = False to take the five-launch layer")
        return out_ids[:, :L + n_done].clone(), hidden[:, :T + n_done - 1].clone()

    def _persistent_cache(self, B, tmax):
        key = (B, tmax)
        c = self._caches.get(key)
        if c is None:
            if len(self._caches) >= 4:   # a few shapes at most stay resident (7B, B=64, 299 positions: 10 GB)
                old = next(iter(self._caches))
                del self._caches[old]
                self._graphs = {k: v for k, v in self._graphs.items() if k[-2:] != old}
            c = self._caches[key] = self.llm.new_cache(B, tmax)
            dev, i64, i32 = self.device, torch.int64, torch.int32
            # generate()'s per-row state, persistent so that the decode hipGraph can address it (ops.decode_book)
            c["book"] = {"forced": torch.zeros((B, tmax), dtype=i64, device=dev), "use_forced": torch.zeros((1,), dtype=i32, device=dev),
                         "steps": torch.zeros((B,), dtype=i32, device=dev), "finished": torch.zeros((B,), dtype=torch.uint8, device=dev),
                         "out_ids": torch.zeros((B, tmax), dtype=i64, device=dev), "lens": torch.zeros((B,), dtype=i64, device=dev),
                         "t_rows": torch.zeros((B,), dtype=i32, device=dev), "tok": torch.zeros((B,), dtype=i64, device=dev),
                         "pos": c["pos"], "nk": c["nk"],
                         "hidden": torch.zeros((B, tmax, self.cfg.llm.hidden), dtype=self.dtype, device=dev)}
        c["len"] = 0
        return c

    def _prefix_cache(self, F, tmax):
        """K / V of the prompt prefix that the rows of a frame share: [F, tmax, H] per layer, the source of ops.kv_prefix_broadcast.
        No decode state hangs on it; the last two shapes stay resident (7B, 8 frames, 275 positions: 1.2 GB)."""
        key = (F, tmax)
        c = self._prefix_caches.pop(key, None)
        if c is None:
            if len(self._prefix_caches) >= 2:
                del self._prefix_caches[next(iter(self._prefix_caches))]
            c = self.llm._new_cache(F, tmax)
        self._prefix_caches[key] = c
        c["len"] = 0
        return c

    def _decode_book_eager(self, cache):
        st = cache["book"]
        B = st["tok"].shape[0]
        x1 = self.llm.embed.index_select(0, st["tok"]).view(B, 1, -1)
        h1 = self.llm.decode_rows(x1, cache)
        logits = self.llm.next_token_logits(h1[:, -1])
        ops.decode_book(ops.argmax_rows(logits), st, h1.reshape(B, -1), self.cfg.pad_token_id, self.cfg.eos_token_id)

    def _decode_book_step(self, cache):
        """One greedy step of generate(): the token written last (cache["book"]["tok"]) is decoded at each row's position and
        the next token is chosen and filed — ONE hipGraph replay per step (per (batch, capacity): the per-row state lives in
        device memory), nothing else on the stream. The first step of a new shape runs eagerly (it is the warm-up of the
        lazily built state inside the ops) and is followed by the capture, which executes nothing."""
        if not self.decode_graphs:
            return self._decode_book_eager(cache)
        key = ("book", self.llm.decode_chain, cache["book"]["tok"].shape[0], cache["tmax"])   # (the last two: what _persistent_cache evicts by)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 16:
                self._graphs.clear()
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            self._decode_book_eager(cache)
            torch.cuda.current_stream(self.device).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool, capture_error_mode="thread_local"):
                self._decode_book_eager(cache)
            self._graphs[key] = g
            return
        g.replay()

    def _decode_step_eager(self, nxt, cache):
        B = nxt.shape[0]
        x1 = self.llm.embed.index_select(0, nxt).view(B, 1, -1)
        h1 = self.llm.decode_rows(x1, cache)
        logits = self.llm.next_token_logits(h1[:, -1])
        return h1, ops.argmax_rows(logits)

    def _decode_step(self, nxt, cache):
        """One greedy step: embed(nxt) -> the layers against the KV cache at each row's own position -> logits -> argmax,
        then every row's position advances by one. Returns (hidden [B,1,H], next ids [B]). The per-row positions live in
        device memory (cache["pos"], cache["nk"]), so ONE hipGraph per (batch, cache capacity) serves every step."""
        if not self.decode_graphs:
            out = self._decode_step_eager(nxt, cache)
        else:
            B = nxt.shape[0]
            key = (self.llm.decode_chain, B, cache["tmax"])
            ent = self._graphs.get(key)
            if ent is None:
                if len(self._graphs) >= 16:
                    self._graphs.clear()
                if self._graph_pool is None:
                    self._graph_pool = torch.cuda.graph_pool_handle()
                static_in = nxt.clone()
                # warm-up outside the capture (lazy one-time work inside the ops); it rewrites this step's K/V slots only
                self._decode_step_eager(static_in, cache)
                torch.cuda.current_stream(self.device).synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._graph_pool, capture_error_mode="thread_local"):
                    h1, out = self._decode_step_eager(static_in, cache)
                ent = self._graphs[key] = (g, static_in, h1, out)
            g, static_in, h1, out = ent
            static_in.copy_(nxt)
            g.replay()
            # outputs are the graph's static tensors: hand out copies so the next replay cannot overwrite them
            out = (h1.clone(), out.clone())
        cache["pos"].add_(1)
        cache["nk"].add_(1)
        return out

    # ---- a10: SAM image encoder --------------------------------------------------------------------------
    @contextlib.contextmanager
    def _chunk_cap(self, n, frames):
        """Encoder chunk n of a `frames`-frame step: the persistent GEMM launches enqueued inside take `sam_chunk_caps[n]`
        workgroups instead of one per CU (ops.gemm_stream_cap on the stream they are enqueued on), leaving CUs to the other stream's kernels. None: no cap;
        "auto": overlap.plan, decided per evaluate() call."""
        caps = self._plan[0]
        cap = caps[min(n, len(caps) - 1)] if caps and self.overlap_streams else 256
        if cap == 256:
            yield
            return
        old = ops.gemm_stream_cap(cap)
        try:
            yield
        finally:
            ops.gemm_stream_cap(old)

    def _chunk(self, frames):
        """Frames per encoder launch sequence: `sam_chunk`, or the plan's choice for sam_chunk="auto"."""
        c = self._plan[2] if self.sam_chunk == "auto" else self.sam_chunk
        return int(c) if c else max(1, min(int(frames), 8))

    def _encoder_passes(self, F, rows_of):
        """The ViT over F frames in passes of `_chunk(F)` frames; rows_of(i, n) -> the patch rows of frames i .. i+n. Every pass
        writes its slice of ONE embedding tensor (torch.cat of four 67 MB pieces was 0.7 ms at the end of the encoder)."""
        enc = self.sam_encoder
        ch = self._chunk(F)
        emb = torch.empty((F, enc.cfg.grid ** 2, enc.cfg.out_chans), dtype=torch.float32 if enc.emb_f32 else enc.dtype, device=self.device) \
            if F > ch else None
        for n, i in enumerate(range(0, F, ch)):
            k = min(ch, F - i)
            with self._chunk_cap(n, F):
                y = enc.forward_rows(rows_of(i, k), k, out=None if emb is None else emb[i:i + k])
        return y if emb is None else emb

    @torch.no_grad()
    def get_visual_embs(self, images):
        """LISA.py:157-168 without the per-image python loop; chunked to bound activation memory."""
        enc = self.sam_encoder
        return self._encoder_passes(images.shape[0], lambda i, k: enc.patch_rows_from_nchw(images[i:i + k].to(self.device, enc.dtype)))

    @torch.no_grad()
    def get_visual_embs_u8(self, frames, mean, std):
        enc = self.sam_encoder
        return self._encoder_passes(frames.shape[0], lambda i, k: enc.patch_rows_from_u8(frames[i:i + k], mean, std))

    @torch.no_grad()
    def get_visual_embs_frames(self, frames, mean, std):
        """A list of uint8 HWC frames of DIFFERENT sizes (a directory of images): each goes through its own Pillow-exact
        resize + fused normalise/pad/patchify (cheap, HBM-bound), the patch rows are concatenated and the ViT runs batched."""
        ing, enc = self.frame_ingest(), self.sam_encoder
        outs = []
        ch = self._chunk(len(frames))
        for n, i in enumerate(range(0, len(frames), ch)):
            rows = []
            for fr in frames[i:i + ch]:
                u8, _ = ing.sam_frames(fr.to(self.device)[None], self.cfg.sam.img_size)
                rows.append(enc.patch_rows_from_u8(u8, mean, std))
            with self._chunk_cap(n, len(frames)):
                outs.append(enc.forward_rows(torch.cat(rows, 0) if len(rows) > 1 else rows[0], len(rows)))
        return torch.cat(outs, 0) if len(outs) > 1 else outs[0]

    # ---- a9: [SEG] gather + text_hidden_fcs ---------------------------------------------------------------
    def seg_embeddings(self, output_ids, hidden):
        mask = output_ids[:, 1:] == self.seg_token_idx
        mask = torch.cat([torch.zeros((mask.shape[0], N_IMG_PAD), dtype=torch.bool, device=mask.device), mask], dim=1)
        assert mask.shape[1] == hidden.shape[1], (mask.shape, hidden.shape)
        counts = mask.int().sum(-1)
        b_idx, t_idx = mask.nonzero(as_tuple=True)
        if b_idx.numel() == 0:
            return torch.empty((0, self.cfg.out_dim), dtype=self.tail_dtype, device=self.device), b_idx, counts
        if self.load_in_8bit:
            # text_hidden_fcs run over every row of each frame (LISA.py:470), one segment per frame's valid rows; the [SEG] rows'
            # f16 outputs are then widened to fp32 for the tail
            B, Th, H = hidden.shape
            x = hidden.reshape(B * Th, H).contiguous()
            # each frame's own rows (the reference generates one frame per call and stops at its EOS): output_ids is left-aligned per
            # row, real prompt then the generated tokens, pad behind a finished row's EOS — its ids up to the last non-pad one, of
            # which the image sentinel stands for 256 hidden rows and the last token has none
            ids_real = output_ids != self.cfg.pad_token_id
            pos = torch.arange(output_ids.shape[1], device=output_ids.device)
            n_ids = torch.where(ids_real, pos[None, :] + 1, torch.zeros_like(pos)[None, :]).amax(1)
            valid = (n_ids + N_IMG_PAD - 1).clamp(max=Th).to(torch.int32)
            q = ops.int8_quantize_act(x, self.llm_int8_threshold, Th, valid)
            h = ops.linear_int8(q, self.fc0[0].cb, self.fc0[0].scb, bias=self.fc0[1], act=ops.ACT_RELU)
            q = ops.int8_quantize_act(h, self.llm_int8_threshold, Th, valid)
            y = ops.linear_int8(q, self.fc2[0].cb, self.fc2[0].scb, bias=self.fc2[1])
            return y.view(B, Th, -1)[b_idx, t_idx].to(self.tail_dtype).contiguous(), b_idx, counts
        rows = hidden[b_idx, t_idx].to(self.tail_dtype).contiguous()
        h = ops.linear(rows, self.fc0[0], bias=self.fc0[1], act=ops.ACT_RELU)
        return ops.linear(h, self.fc2[0], bias=self.fc2[1]), b_idx, counts

    def frame_ingest(self):
        """Device-side host preprocessing (rows a1/a2): Pillow-exact resizes + CLIP normalisation on uint8 frames."""
        if self._ingest is None:
            from .preprocess import FrameIngest
            self._ingest = FrameIngest(self.device)
        return self._ingest

    # ---- the boundary --------------------------------------------------------------------------------------
    @staticmethod
    def _check_grouped(offset, images_clip, images, input_ids, resize_list, original_size_list, frames_u8, attention_mask, forced_answer):
        """evaluate(offset=)'s arguments, checked on the host before anything is enqueued: -> (frame_of int32 [B] on the CPU, F).
        A ValueError names the argument that does not fit."""
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2:
            raise ValueError("input_ids: a [B, L] tensor of prompt rows is expected with offset=")
        B = input_ids.shape[0]
        counts = {name: len(v) for name, v in (("images_clip", images_clip), ("frames_u8", frames_u8), ("images", images),
                                               ("resize_list", resize_list), ("original_size_list", original_size_list)) if v is not None}
        if not any(n in counts for n in ("images_clip", "frames_u8", "images")):
            raise ValueError("images / frames_u8: evaluate() needs the frames")
        F = counts.get("images_clip", counts.get("frames_u8", counts.get("images")))
        for name, n in counts.items():
            if n != F:
                raise ValueError(f"{name}: {n} entries, but the call has {F} frames (per-frame inputs have one entry per frame with offset=)")
        if attention_mask is not None and tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"attention_mask: shape {tuple(attention_mask.shape)}, input_ids has {tuple(input_ids.shape)}")
        if forced_answer is not None and forced_answer.shape[0] != B:
            raise ValueError(f"forced_answer: {forced_answer.shape[0]} rows, input_ids has {B}")
        return prompt_groups.check_offset(offset, B, F), F

    @torch.no_grad()
    def evaluate(self, images_clip, images, input_ids, resize_list, original_size_list, max_new_tokens=32,
                 tokenizer=None, forced_answer=None, frames_u8=None, attention_mask=None, *, offset=None):
        """offset (keyword only; int64 [F+1], the convention of the reference's model_forward, LISA.py:224-262): several prompt rows
        per frame. images_clip / images / frames_u8 / resize_list / original_size_list then have F entries, input_ids / attention_mask
        / forced_answer B = offset[-1] rows, and row b belongs to frame f where offset[f] <= b < offset[f+1] (a frame without rows is
        encoded and unused). Everything that does not depend on the prompt runs once per frame: the SAM encoder, the CLIP tower, the
        projector and — when the rows share their ids up to and past the <image> sentinel — the Llama prefill of that prefix
        (generate(frame_of=)). Returns are per prompt row, as without offset. None, or arange(B+1): one frame per row, the plain path."""
        frame_of, n_frames = None, input_ids.shape[0]
        if offset is not None:
            frame_of, n_frames = self._check_grouped(offset, images_clip, images, input_ids, resize_list, original_size_list, frames_u8,
                                                     attention_mask, forced_answer)
            if prompt_groups.is_identity(offset):
                frame_of = None
        if frame_of is None:
            self.last_group_plan = {"frames": n_frames, "rows": n_frames, "shared_prefix_ids": 0, "prefix_positions": 0, "shared": False,
                                    "encoder_frames": n_frames}
        # The SAM encoder (MFMA-bound, ~60 % of the FLOPs) does not depend on the language model: it runs on its own
        # HIP stream so its big GEMMs fill the CUs while the HBM/latency-bound greedy decode steps of the LLM trickle
        # through on the caller's stream. Joined before the mask decoders.
        cur = torch.cuda.current_stream(self.device)
        side = self._sam_stream if self.overlap_streams else cur
        frame_list = isinstance(frames_u8, (list, tuple))   # frames of different sizes: one [H,W,3] uint8 tensor each
        if frames_u8 is not None:
            if not frame_list:
                frames_u8 = frames_u8.to(self.device)
            if images_clip is None:   # a2 on the device: CLIPImageProcessor.preprocess of the same uint8 frames
                ing = self.frame_ingest()
                if frame_list:
                    images_clip = torch.cat([ing.clip_pixels(f.to(self.device)[None], self.cfg.clip.image, self.dtype)
                                             for f in frames_u8], 0)
                else:
                    images_clip = ing.clip_pixels(frames_u8, self.cfg.clip.image, self.dtype)
        inputs_ready = torch.cuda.Event()
        inputs_ready.record(cur)
        sam_out = []

        def launch_sam():
            side.wait_event(inputs_ready)
            if late and wait:   # really BEHIND the prefill on the GPU too, not only in the host's enqueue order
                ev = torch.cuda.Event()
                ev.record(cur)
                side.wait_event(ev)
            with torch.cuda.stream(side):
                if frames_u8 is not None:
                    from .preprocess import SAM_MEAN, SAM_STD
                    # a1 on the device: ResizeLongestSide (identity when the long side is img_size), then the fused
                    # normalise + pad + patchify of haff_patchify_u8
                    if frame_list:
                        sam_out.append(self.get_visual_embs_frames(frames_u8, SAM_MEAN, SAM_STD))
                    else:
                        sam_u8, _ = self.frame_ingest().sam_frames(frames_u8, self.cfg.sam.img_size)
                        sam_out.append(self.get_visual_embs_u8(sam_u8, SAM_MEAN, SAM_STD))
                else:
                    sam_out.append(self.get_visual_embs(images))

        # Where the encoder is enqueued. Throughput batches: first, so its GEMMs run beside the CLIP tower and the prefill.
        # A few frames (latency): behind the prefill, so it runs beside the HBM-bound decode steps, which leave the matrix
        # cores idle, instead of time-slicing them with the prefill (and the host enqueues it while the prefill runs).
        # (round 5, bench.py --sam-beside-decode on / off at 8 and 16 frames: behind the prefill is +0.4 ... +1.8 % for 7B and 13B there
        # too; at 64 frames the encoder is 60 % of the step and has to start first)
        late = self.overlap_streams and self.sam_beside_decode is not False and \
            (self.sam_beside_decode is True or n_frames <= 16)
        # Which kernels decode: a function of the BATCH alone, never of the schedule (every schedule of one batch must give the same
        # bits: tests/test_lisa_gpu.py::test_stream_schedules_do_not_change_results, tools/two_stream_soak.py). "auto": the chained
        # launch below overlap.MIN_FRAMES frames — where no encoder pass is ever capped beside the decode steps — five launches per
        # layer from there on (the plan caps the encoder beside them; a chained step would starve it: the comment at decode_chain).
        n_rows = input_ids.shape[0]
        chain_now = bool(self.llm.decode_chain) and n_rows <= self.llm.carry_rms_max_rows and \
            (self.decode_chain is True or (self.decode_chain == "auto" and n_rows < overlap.MIN_FRAMES))
        if chain_now and self.decode_chain == "auto" and self.sam_beside_decode is None:
            # chained decode steps: the encoder FIRST (beside CLIP + prefill), the steps alone behind it — a chained step is one 3 ms
            # launch whose workgroups hold every CU, the encoder's launches cannot slip in between (same box, one frame: encoder
            # first + chain 40.6 ms, behind the prefill + five launches 41.3, behind the prefill + chain 41.8-42.1)
            late = False
        # ... and which CUs its GEMM launches leave to the decode steps (overlap.py), for the frames that are encoded (with offset=: F, not
        # the number of prompt rows)
        chunk = overlap.auto_chunk(n_frames, late) if self.sam_chunk == "auto" else self.sam_chunk
        caps, wait = None, False
        if self.overlap_streams:
            if self.sam_chunk_caps == "auto":
                # the work model's rates follow THIS device (two timed probes, once per process: overlap.calibrate)
                rates = overlap.calibrate(self.device) if self.calibrate_overlap and n_frames >= overlap.MIN_FRAMES else overlap.NOMINAL
                self.last_rates = rates
                caps, wait = overlap.plan(self.cfg, n_frames, chunk, input_ids.shape[1],
                                          min(max_new_tokens, self.expected_new_tokens), late, rates)
            elif self.sam_chunk_caps:
                caps, wait = list(self.sam_chunk_caps), late
            if self.sam_waits_for_prefill != "auto":
                wait = bool(self.sam_waits_for_prefill) and late
        self._plan = self.last_plan = (caps, wait, chunk)
        chain_prev = self.llm.decode_chain
        self.llm.decode_chain = chain_prev if chain_now else False
        self.last_decode_chain = chain_now
        if not late:
            launch_sam()
        try:
            output_ids, hidden = self.generate(images_clip, input_ids, max_new_tokens, forced_answer, attention_mask,
                                               after_prefill=launch_sam if late else None, needed_hidden_only=True, frame_of=frame_of)
        finally:
            self.llm.decode_chain = chain_prev
        emb = sam_out[0]
        self._plan = (None, False, chunk)     # the encoder is enqueued: direct get_visual_embs* calls take no caps
        pred, frame_idx, counts = self.seg_embeddings(output_ids, hidden)
        if frame_of is not None:
            # prompt rows -> their frames: the embedding the mask decoders gather, and the sizes each row's masks are restored to
            frame_idx = frame_of.to(self.device).long().index_select(0, frame_idx)
            resize_list = [resize_list[f] for f in frame_of.tolist()]
            original_size_list = [original_size_list[f] for f in frame_of.tolist()]
        cur.wait_stream(side)
        emb.record_stream(cur)
        B = output_ids.shape[0]
        pred_masks_left, pred_masks_right, taxonomies = [], [], []
        if pred.shape[0] > 1 and self.tail_per_row:
            parts = [self._decoder_tail(emb, frame_idx[i:i + 1], pred[i:i + 1]) for i in range(pred.shape[0])]
            lo_l, lo_r, tax = (torch.cat(p, 0) for p in zip(*parts))
        elif pred.shape[0] > 0:
            lo_l, lo_r, tax = self._decoder_tail(emb, frame_idx, pred)
        offs = torch.cat([torch.zeros(1, dtype=torch.long), counts.cpu().long().cumsum(0)]).tolist()
        # frames of one size (a batch of equally sized frames: the throughput case): ONE postprocess launch per hand over all
        # prompts, sliced per frame below, instead of two launches per frame
        same = pred.shape[0] > 0 and all(tuple(r) == tuple(resize_list[0]) for r in resize_list) and \
            all(tuple(o) == tuple(original_size_list[0]) for o in original_size_list)
        if same:
            post_l = self.sam_decoder.postprocess(lo_l.contiguous(), resize_list[0], original_size_list[0])
            post_r = self.sam_decoder.postprocess(lo_r.contiguous(), resize_list[0], original_size_list[0])
        for i in range(B):
            a, b = offs[i], offs[i + 1]
            if same and b > a:
                pred_masks_left.append(post_l[a:b])
                pred_masks_right.append(post_r[a:b])
                taxonomies.append(tax[a:b])
                continue
            if b == a:
                h0, w0 = original_size_list[i]
                pred_masks_left.append(torch.empty((0, h0, w0), dtype=torch.float32, device=self.device))
                pred_masks_right.append(torch.empty((0, h0, w0), dtype=torch.float32, device=self.device))
                taxonomies.append(torch.empty((0, 4), dtype=torch.float32, device=self.device))
                continue
            pred_masks_left.append(self.sam_decoder.postprocess(lo_l[a:b].contiguous(), resize_list[i], original_size_list[i]))
            pred_masks_right.append(self.sam_decoder.postprocess(lo_r[a:b].contiguous(), resize_list[i], original_size_list[i]))
            taxonomies.append(tax[a:b])
        return output_ids, pred_masks_left, pred_masks_right, taxonomies

    predict = evaluate

    def _replay(self, key, fn, inputs):
        """fn(*static inputs) -> tuple of tensors, as ONE hipGraph per key (a few frames: these stages are ~150-190 small
        launches each and the host, not the GPU, sets their pace). First use runs eagerly (warm-up and result), then captures."""
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= 16:
                self._graphs.clear()
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            static = [t.clone() for t in inputs]
            out = fn(*static)
            torch.cuda.current_stream(self.device).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool, capture_error_mode="thread_local"):
                outs = fn(*static)
            self._graphs[key] = (g, static, outs)
            return out
        g, static, outs = ent
        for dst, src in zip(static, inputs):
            dst.copy_(src)
        g.replay()
        return tuple(o.clone() for o in outs)

    def _decoder_tail(self, emb, frame_idx, pred):
        """Prompt encoder + both two-way mask decoders -> (low-res left, low-res right, taxonomy)."""
        fn = lambda e, i, t: tuple(self.sam_decoder.decode(e, i, t)[:3])   # noqa: E731
        if not self.decode_graphs or pred.shape[0] > 8 or emb.shape[0] > 8:
            return fn(emb, frame_idx, pred)
        return self._replay(("tail", emb.shape[0], pred.shape[0], emb.dtype), fn, [emb, frame_idx, pred])

    def eval(self):
        return self

    @classmethod
    def from_state_dict(cls, cfg, state_dict, dtype=torch.bfloat16, device="cuda:0", **kw):
        return cls(cfg, state_dict, dtype=dtype, device=device, **kw)

    @staticmethod
    def read_lora_checkpoint(path, load_in_4bit=True):
        """The trained tensors of train_ds.py's latest.pt for lora_state=: an NF4 fine-tune's (`base_format` "nf4") only. Adapters
        fitted on a 16-bit base, and any checkpoint without load_in_4bit, are refused by name: those are served merged."""
        if not load_in_4bit:
            raise ValueError(f"lora_checkpoint={path!r} needs load_in_4bit=True: unmerged adapters are served on the NF4 base only; "
                             "16-bit bases are served merged (merge_lora.py)")
        blob = torch.load(path, map_location="cpu", weights_only=False)
        if not (isinstance(blob, dict) and "params" in blob):
            raise ValueError(f"lora_checkpoint={path!r} is not a train_ds.py checkpoint (no 'params' entry)")
        if blob.get("base_format") != "nf4":
            raise ValueError(f"lora_checkpoint={path!r} has base_format={blob.get('base_format')!r}: its adapters were fitted on a "
                             "16-bit base, not on the NF4 codes (train_ds.py --load_in_4bit); merge it with merge_lora.py instead")
        return blob["params"]

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, vision_tower=None, seg_token_idx=None,
                        torch_dtype=torch.bfloat16, sam_checkpoint=None, device="cuda:0", lora_checkpoint=None, **kw):
        """The constructor the reference's CLIs use (inference.py:158-168, chat.py:104-114):
        `LISAForCausalLM.from_pretrained(version, vision_tower=, seg_token_idx=, torch_dtype=)` followed by
        `initialize_vision_modules` — a merged checkpoint directory (merge_lora_weights_and_save_hf_model.py:149-155 layout:
        sharded weights + index + config.json, `vision_tower` keys excluded) plus the CLIP tower from its own directory
        (clip_encoder.py:21-29). Local directories only: there is no hub access in this setting."""
        from . import checkpoint
        if lora_checkpoint is not None:
            kw["lora_state"] = cls.read_lora_checkpoint(lora_checkpoint, kw.get("load_in_4bit", False))
        cfg = checkpoint.config_from_dir(pretrained_model_name_or_path)
        if seg_token_idx is not None:
            cfg.seg_token_idx = int(seg_token_idx)
        sd = checkpoint.load_state_dict(pretrained_model_name_or_path, vision_tower, sam_checkpoint, cfg=cfg)
        # The reference takes [SEG] / <im_start> / <im_end> from the TOKENIZER (inference.py:115-131, train_ds.py:142-149); here, in
        # order of authority: the directory's added_tokens.json; else the three rows behind the sentencepiece vocabulary when the
        # embedding has exactly base + 3 rows; else (directories without tokenizer files: this repo's synthetic checkpoints) the
        # last three rows when the embedding has config.json's vocab_size or vocab_size + 3 rows. Anything else — a plain base
        # without the added rows, a vocabulary padded to a multiple of 64 — is refused instead of silently reading ordinary or
        # padding rows as [SEG]. An explicit seg_token_idx is kept as given.
        rows = sd["model.embed_tokens.weight"].shape[0]
        ids = checkpoint.resolve_added_tokens(pretrained_model_name_or_path, rows, layout_asserted=seg_token_idx is not None)
        cfg.llm.vocab = rows
        cfg.im_start_idx, cfg.im_end_idx = int(ids["<im_start>"]), int(ids["<im_end>"])
        if seg_token_idx is None:
            cfg.seg_token_idx = int(ids["[SEG]"])
        return cls(cfg, sd, dtype=torch_dtype, device=device, **kw)
