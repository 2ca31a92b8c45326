"""The fp16 inference mode end to end (LisaMI355(dtype=torch.float16)) against the CPU oracle and beside the bf16 mode.

One weight set serves all three precisions: bf16-rounded values with every |w| < 2^-14 set to zero are exact in bf16, fp16 (normal
range, 11 significand bits) and fp32, and so are the inputs. fp16 operands carry three more significand bits than bf16, so every
rounding of an MFMA operand is 8x smaller: the fp16 mode must land at most half as far from the oracle as the bf16 mode on the
same inputs, and decide no more mask pixels differently."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _exact_in_all(t):
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def _setup(cfg_name, seed=5, B=2, n_gen=4, prompt_len=8):
    import haff  # noqa: F401
    from haff import config as hcfg
    from haff import weights as hw
    cfg = getattr(hcfg, cfg_name)()
    sd = {k: _exact_in_all(v) if torch.is_floating_point(v) else v for k, v in hw.make_state_dict(cfg, seed).items()}
    rng = np.random.default_rng(seed + 7)
    S = cfg.sam.img_size
    images = _exact_in_all(torch.from_numpy(rng.standard_normal((B, 3, S, S), dtype=np.float32)))
    images_clip = _exact_in_all(torch.from_numpy(rng.standard_normal((B, 3, cfg.clip.image, cfg.clip.image), dtype=np.float32)))
    text = torch.from_numpy(rng.integers(3, cfg.llm.vocab - 3, size=(B, prompt_len))).long()
    ids = torch.cat([torch.tensor([[cfg.bos_token_id, cfg.im_start_idx, -200, cfg.im_end_idx]]).expand(B, -1), text], 1)
    forced = torch.from_numpy(rng.integers(3, cfg.llm.vocab - 3, size=(B, n_gen))).long()
    forced[:, 1] = cfg.seg_token_idx
    forced[:, -1] = cfg.eos_token_id
    return cfg, sd, images, images_clip, ids, forced


def _iou(a, b):
    inter = (a & b).sum().item()
    union = (a | b).sum().item()
    return inter / union if union else 1.0


def _run(model, dev, images_clip, images, ids, forced, resize, orig):
    out = model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), resize, orig, max_new_tokens=forced.shape[1],
                         forced_answer=forced)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cfg_name", ["tiny", "mid"])
def test_fp16_mode_is_closer_to_the_oracle_than_bf16(dev, cfg_name):
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip, ids, forced = _setup(cfg_name)
    S = cfg.sam.img_size
    B = ids.shape[0]
    resize = [(S, S), (S, S - 32)]
    orig = [(S, S), (S // 2 + 3, S // 2 - 10)]
    with torch.no_grad():
        ref_ids, ref_l, ref_r, ref_t = O.lisa_evaluate(sd, cfg, images_clip, images, ids, resize, orig,
                                                       max_new_tokens=forced.shape[1], forced_answer=forced, use_cache=False)
    stats = {}
    for dt in (torch.bfloat16, torch.float16):
        model = LisaMI355(cfg, sd, dtype=dt, device=dev)
        out_ids, left, right, tax = _run(model, dev, images_clip, images, ids, forced, resize, orig)
        errs, ious, terrs = [], [], []
        for i in range(B):
            for got, ref in ((left[i], ref_l[i]), (right[i], ref_r[i])):
                g = got.cpu()
                assert torch.isfinite(g).all()
                errs.append((g - ref).abs().max().item() / ref.abs().max().item())
                ious.append(_iou(g > 0, ref > 0))
            terrs.append((tax[i].cpu() - ref_t[i]).abs().max().item())
        stats[dt] = (out_ids.cpu(), max(errs), min(ious), max(terrs))
        print(f"{cfg_name} {dt}: max err/scale {max(errs):.3e}, min IoU {min(ious):.5f}, taxonomy err {max(terrs):.3e}")
        del model
    ids16, err16, iou16, terr16 = stats[torch.float16]
    _, err_bf, iou_bf, _ = stats[torch.bfloat16]
    assert torch.equal(ids16, ref_ids)
    assert err16 <= 0.5 * err_bf, (err16, err_bf)
    assert iou16 >= iou_bf, (iou16, iou_bf)
    assert terr16 <= 1e-3


def test_fp16_image_embedding_is_closer_than_bf16(dev):
    """The ViT-H stack (fp16 activations, f32 neck) against the oracle's image encoder: a smaller rms error than the bf16 mode's."""
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip, ids, forced = _setup("mid")
    with torch.no_grad():
        ref = O.sam_image_encoder(sd, "model.visual_model.image_encoder", images, cfg.sam).float()
    rms = {}
    for dt in (torch.bfloat16, torch.float16):
        model = LisaMI355(cfg, sd, dtype=dt, device=dev)
        emb = model.sam_encoder(images.to(dev)).float().cpu()
        torch.cuda.synchronize()
        ref_cl = ref.permute(0, 2, 3, 1).reshape(emb.shape)   # oracle [B, C, g, g] -> the encoder's channels-last [B, g*g, C]
        rms[dt] = ((emb - ref_cl).pow(2).mean().sqrt() / ref_cl.pow(2).mean().sqrt()).item()
        del model
    print(f"image embedding rel rms error: bf16 {rms[torch.bfloat16]:.3e}, fp16 {rms[torch.float16]:.3e}")
    assert rms[torch.float16] < rms[torch.bfloat16]


def test_fp16_runs_are_repeatable_and_schedule_independent(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = _setup("tiny", B=1)
    S = cfg.sam.img_size
    resize, orig = [(S, S)], [(S, S)]
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev)
    assert model.fp32_tail and model.sam_encoder.neck_f32 and model.llm.decode_chain is False
    first = _run(model, dev, images_clip, images, ids, forced, resize, orig)
    assert model.last_decode_chain is False        # one frame: the chained step is a bf16 kernel, fp16 takes five launches
    runs = [_run(model, dev, images_clip, images, ids, forced, resize, orig)]
    model.overlap_streams = False
    runs.append(_run(model, dev, images_clip, images, ids, forced, resize, orig))
    model.overlap_streams = True
    model.decode_graphs = False
    runs.append(_run(model, dev, images_clip, images, ids, forced, resize, orig))
    for r in runs:
        assert torch.equal(r[0], first[0])
        for a, b in zip(r[1] + r[2] + r[3], first[1] + first[2] + first[3]):
            assert torch.equal(a, b)


def test_fp16_refuses_bf16_only_options(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = _setup("tiny", B=1)
    for kw in ({"fp32_stream": True}, {"fp32_stream": "sam"}, {"neck_f32": True}, {"fp32_tail": False}):
        with pytest.raises(ValueError):
            LisaMI355(cfg, sd, dtype=torch.float16, device=dev, **kw)
    big = dict(sd)
    big["lm_head.weight"] = big["lm_head.weight"].clone()
    big["lm_head.weight"][0, 0] = 1e5
    with pytest.raises(ValueError, match="lm_head.weight"):
        LisaMI355(cfg, big, dtype=torch.float16, device=dev)
    tiny_w = dict(sd)
    tiny_w["lm_head.weight"] = tiny_w["lm_head.weight"].clone()
    tiny_w["lm_head.weight"][0, :3] = 1e-9
    with pytest.warns(UserWarning, match="3 nonzero weights flushed"):
        model = LisaMI355(cfg, tiny_w, dtype=torch.float16, device=dev)
    assert model.fp16_flushed_weights == 3
    model.llm.decode_chain = True
    with pytest.raises(ValueError, match="decode_chain"):
        model.llm.decode_rows(torch.zeros((1, 1, cfg.llm.hidden), dtype=torch.float16, device=dev), model.llm.new_cache(1, 16))
