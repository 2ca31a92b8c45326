"""LisaMI355.evaluate(offset=): several prompt rows on one frame, on the MI355X. The grouped call — encoders once per frame, the prompts'
common prefix prefilled once per frame and its K / V broadcast (haff_kv_prefix_broadcast), the rows' own ids prefilled behind it —
against one batch-1 evaluate() per (prompt, its frame) pair. The bars are those of test_lisa_gpu.py::test_ragged_prompts_equal_batch1_runs:
the substitution is of the same kind (the same rows through differently shaped launches)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TAILS = (3, 9, 6, 4, 7)


def _setup(mode, n_frames, seed=5):
    import haff  # noqa: F401
    from haff import config as hcfg
    from haff import weights as hw
    cfg = hcfg.tiny()
    sd = hw.make_state_dict(cfg, seed)
    rng = np.random.default_rng(seed + 7)
    S = cfg.sam.img_size
    images = torch.from_numpy(rng.standard_normal((n_frames, 3, S, S), dtype=np.float32))
    images_clip = torch.from_numpy(rng.standard_normal((n_frames, 3, cfg.clip.image, cfg.clip.image), dtype=np.float32))
    if mode != "f32":
        hw.round_to_bf16_(sd)
        images = images.to(torch.bfloat16).float()
        images_clip = images_clip.to(torch.bfloat16).float()
    return cfg, sd, images, images_clip


def _head(cfg):
    return [cfg.bos_token_id, cfg.im_start_idx, -200, cfg.im_end_idx]


def _pad(cfg, prompts):
    L = max(len(p) for p in prompts)
    ids = torch.full((len(prompts), L), cfg.pad_token_id, dtype=torch.long)
    mask = torch.zeros((len(prompts), L), dtype=torch.bool)
    for b, p in enumerate(prompts):
        ids[b, :len(p)] = torch.tensor(p)
        mask[b, :len(p)] = True
    return ids, mask


def _prompts(cfg, tails, seed=11):
    rng = np.random.default_rng(seed)
    return [_head(cfg) + rng.integers(3, 300, size=n).tolist() for n in tails]


def _forced(cfg):
    """[SEG] at a different generated index per row; row 1 ends early with EOS; row 3 has no [SEG]"""
    seg, eos = cfg.seg_token_idx, cfg.eos_token_id
    return torch.tensor([[7, seg, 9, 11, eos],
                         [seg, 8, eos, 0, 0],
                         [5, 6, 7, seg, eos],
                         [4, 5, 6, 7, eos],
                         [9, 9, seg, eos, 0]])


def _compare(mode, cfg, grouped, singles, oracles=None):
    """grouped: evaluate(offset=)'s tuple over B rows; singles[b]: the batch-1 tuple of row b on its own frame"""
    bo, bl, br, bt = grouped
    for b, (o, l, r, t) in enumerate(singles):
        n = o.shape[1]
        assert torch.equal(bo[b, :n].cpu(), o[0].cpu()) and bool((bo[b, n:] == cfg.pad_token_id).all()), b
        for side, got, ref in (("left", bl[b], l[0]), ("right", br[b], r[0])):
            assert got.shape == ref.shape, (b, side, got.shape, ref.shape)
            if ref.shape[0] == 0:
                continue
            scale = ref.abs().max().item()
            err = (got - ref).abs().max().item()
            print(f"{mode} row{b} {side}: vs batch-1 {err:.2e} (scale {scale:.2f})")
            assert err <= (1e-3 if mode == "f32" else 4e-2 * scale), (b, side, err, scale)
            if oracles is not None:
                orc = oracles[b][1 if side == "left" else 2][0]
                e_or = (got.cpu() - orc).abs().max().item()
                print(f"{mode} row{b} {side}: vs oracle {e_or:.2e}")
                assert got.shape == orc.shape and e_or <= 1e-3, (b, side, e_or)
        assert bt[b].shape == t[0].shape
        if t[0].numel():
            assert (bt[b] - t[0]).abs().max().item() <= (1e-4 if mode == "f32" else 3e-2), b


def _count_encoder_frames(model):
    seen = []
    orig = model.get_visual_embs

    def counted(images):
        seen.append(int(images.shape[0]))
        return orig(images)
    model.get_visual_embs = counted
    return seen


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_grouped_equals_per_pair(dev, mode):
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip = _setup(mode, 2)
    model = LisaMI355(cfg, sd, dtype=torch.float32 if mode == "f32" else torch.bfloat16, device=dev)
    S = cfg.sam.img_size
    prompts = _prompts(cfg, TAILS)
    ids, mask = _pad(cfg, prompts)
    forced = _forced(cfg)
    offset = torch.tensor([0, 3, 5])
    frame_of = [0, 0, 0, 1, 1]
    sizes = [(S, S)] * 2
    seen = _count_encoder_frames(model)
    grouped = model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=5, forced_answer=forced,
                             attention_mask=mask, offset=offset)
    assert seen == [2], seen                               # the SAM encoder saw the 2 frames, not one per prompt
    plan = dict(model.last_group_plan)
    n_img = cfg.clip.n_patches
    assert plan["shared"] is True and plan["encoder_frames"] == 2 and plan["shared_prefix_ids"] == 4
    assert plan["prefix_positions"] == 4 + n_img - 1 and plan["frames"] == 2 and plan["rows"] == 5
    assert grouped[0].shape == (5, ids.shape[1] + 5)
    assert grouped[1][3].shape == (0, S, S) and grouped[2][3].shape == (0, S, S) and grouped[3][3].shape == (0, 4)   # the row without [SEG]
    singles, oracles = [], []
    for b, p in enumerate(prompts):
        f = frame_of[b]
        one = torch.tensor([p])
        singles.append(model.evaluate(images_clip[f:f + 1].to(dev), images[f:f + 1].to(dev), one.to(dev), sizes[:1], sizes[:1],
                                      max_new_tokens=5, forced_answer=forced[b:b + 1]))
        if mode == "f32":
            with torch.no_grad():
                oracles.append(O.lisa_evaluate(sd, cfg, images_clip[f:f + 1], images[f:f + 1], one, sizes[:1], sizes[:1],
                                               max_new_tokens=5, forced_answer=forced[b:b + 1], use_cache=True))
            assert torch.equal(singles[-1][0].cpu(), oracles[-1][0])
    assert model.last_group_plan["shared"] is False and model.last_group_plan["encoder_frames"] == 1
    _compare(mode, cfg, grouped, singles, oracles if mode == "f32" else None)


def test_free_running_greedy_tokens_equal_per_pair(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup("f32", 2)
    model = LisaMI355(cfg, sd, dtype=torch.float32, device=dev)
    S = cfg.sam.img_size
    prompts = _prompts(cfg, TAILS, seed=12)
    ids, mask = _pad(cfg, prompts)
    sizes = [(S, S)] * 2
    bo = model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=6, attention_mask=mask,
                        offset=torch.tensor([0, 3, 5]))[0]
    assert model.last_group_plan["shared"] is True
    for b, p in enumerate(prompts):
        f = 0 if b < 3 else 1
        o = model.evaluate(images_clip[f:f + 1].to(dev), images[f:f + 1].to(dev), torch.tensor([p]).to(dev), sizes[:1], sizes[:1],
                           max_new_tokens=6)[0]
        n = o.shape[1]
        assert n > len(p)
        assert torch.equal(bo[b, :n].cpu(), o[0].cpu()) and bool((bo[b, n:] == cfg.pad_token_id).all()), (b, bo[b].tolist(), o[0].tolist())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_rows_that_differ_before_the_sentinel_take_the_fallback(dev, mode):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup(mode, 1)
    model = LisaMI355(cfg, sd, dtype=torch.float32 if mode == "f32" else torch.bfloat16, device=dev)
    S = cfg.sam.img_size
    prompts = [_head(cfg) + [21, 22, 23, 24, 25], [cfg.bos_token_id, 17, -200, cfg.im_end_idx, 31, 32, 33]]
    ids, mask = _pad(cfg, prompts)
    forced = _forced(cfg)[[0, 2]]
    sizes = [(S, S)]
    seen = _count_encoder_frames(model)
    grouped = model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=5, forced_answer=forced,
                             attention_mask=mask, offset=torch.tensor([0, 2]))
    plan = model.last_group_plan
    assert plan["shared"] is False and plan["encoder_frames"] == 1 and plan["shared_prefix_ids"] == 0 and plan["prefix_positions"] == 0
    assert seen == [1]
    singles = [model.evaluate(images_clip.to(dev), images.to(dev), torch.tensor([p]).to(dev), sizes, sizes, max_new_tokens=5,
                              forced_answer=forced[b:b + 1]) for b, p in enumerate(prompts)]
    _compare(mode, cfg, grouped, singles)


def _bits_equal(a, b):
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert u.shape == v.shape and torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_one_row_per_frame_is_the_plain_path_bit_for_bit(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup("bf16", 3)
    model = LisaMI355(cfg, sd, dtype=torch.bfloat16, device=dev)
    S = cfg.sam.img_size
    ids, mask = _pad(cfg, _prompts(cfg, (3, 9, 6)))
    forced = _forced(cfg)[:3]
    sizes = [(S, S)] * 3
    run = lambda **kw: model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=5,   # noqa: E731
                                      forced_answer=forced, attention_mask=mask, **kw)
    run()                                                  # (the first call of a shape runs its decode step eagerly and captures it)
    plain = run()
    again = run(offset=torch.arange(4))
    plan = model.last_group_plan
    assert plan["shared"] is False and plan["encoder_frames"] == 3 and plan["rows"] == 3
    _bits_equal(plain, again)
    _bits_equal(plain, run(offset=None))


def test_invalid_arguments_raise_before_any_device_work(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup("bf16", 2)
    model = LisaMI355(cfg, sd, dtype=torch.bfloat16, device=dev)
    S = cfg.sam.img_size
    ids, mask = _pad(cfg, _prompts(cfg, (3, 9, 6)))
    sizes = [(S, S)] * 2
    seen = _count_encoder_frames(model)
    model.encode_images = None                             # any device work would fail on this
    args = (images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes)
    for name, a, kw in (("offset", args, {"offset": torch.tensor([0, 2, 1, 3])}),
                        ("offset", args, {"offset": torch.tensor([0, 2, 4])}),
                        ("offset", args, {"offset": torch.tensor([0, 1, 3], dtype=torch.int32)}),
                        ("offset", args, {"offset": torch.tensor([0, 3])}),
                        ("resize_list", args[:3] + (sizes[:1], sizes), {"offset": torch.tensor([0, 1, 3])}),
                        ("original_size_list", args[:4] + (sizes * 2,), {"offset": torch.tensor([0, 1, 3])}),
                        ("images", (args[0], images[:1].to(dev)) + args[2:], {"offset": torch.tensor([0, 1, 3])}),
                        ("attention_mask", args, {"offset": torch.tensor([0, 1, 3]), "attention_mask": mask[:2]})):
        with pytest.raises(ValueError, match=name):
            model.evaluate(*a, max_new_tokens=2, **kw)
    assert seen == []
    with pytest.raises(TypeError):                         # keyword only
        model.evaluate(*args, 2, None, None, None, None, torch.tensor([0, 1, 3]))
    assert model.predict.__func__ is model.evaluate.__func__


def test_frames_of_different_sizes_and_an_empty_frame(dev):
    from haff import preprocess as P
    from haff.lisa import LisaMI355
    cfg, sd, _, _ = _setup("bf16", 1)
    model = LisaMI355(cfg, sd, dtype=torch.float32, device=dev)
    S = cfg.sam.img_size
    rng = np.random.default_rng(3)
    hw_ = [(150, 224), (96, 64), (120, 80)]
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in hw_]
    resize = [P.get_preprocess_shape(h, w, S) for h, w in hw_]
    prompts = _prompts(cfg, (3, 9, 6))
    ids, mask = _pad(cfg, prompts)
    forced = _forced(cfg)[[0, 2, 4]]

    def singles(frame_of):
        return [model.evaluate(None, None, torch.tensor([p]).to(dev), [resize[f]], [hw_[f]], max_new_tokens=5,
                               forced_answer=forced[b:b + 1], frames_u8=[frames[f]]) for b, (p, f) in enumerate(zip(prompts, frame_of))]
    # two frames, rows 0 and 1 on the first
    grouped = model.evaluate(None, None, ids.to(dev), resize[:2], hw_[:2], max_new_tokens=5, forced_answer=forced, attention_mask=mask,
                             frames_u8=frames[:2], offset=torch.tensor([0, 2, 3]))
    assert model.last_group_plan["shared"] is True and model.last_group_plan["encoder_frames"] == 2
    for b, f in enumerate((0, 0, 1)):
        assert grouped[1][b].shape == (1,) + hw_[f] and grouped[2][b].shape == (1,) + hw_[f]
    _compare("f32", cfg, grouped, singles((0, 0, 1)))
    # three frames, the middle one without rows: encoded and unused
    grouped = model.evaluate(None, None, ids.to(dev), resize, hw_, max_new_tokens=5, forced_answer=forced, attention_mask=mask,
                             frames_u8=frames, offset=torch.tensor([0, 2, 2, 3]))
    assert model.last_group_plan["encoder_frames"] == 3 and model.last_group_plan["frames"] == 3
    for b, f in enumerate((0, 0, 2)):
        assert grouped[1][b].shape == (1,) + hw_[f]
    _compare("f32", cfg, grouped, singles((0, 0, 2)))


def _quantised_case(dev, **kw):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup("bf16", 1)
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, **kw)
    S = cfg.sam.img_size
    prompts = _prompts(cfg, (3, 9, 6))
    ids, mask = _pad(cfg, prompts)
    forced = _forced(cfg)[[0, 2, 4]]
    sizes = [(S, S)]
    grouped = model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=5, forced_answer=forced,
                             attention_mask=mask, offset=torch.tensor([0, 3]))
    plan = dict(model.last_group_plan)
    singles = [model.evaluate(images_clip.to(dev), images.to(dev), torch.tensor([p]).to(dev), sizes, sizes, max_new_tokens=5,
                              forced_answer=forced[b:b + 1]) for b, p in enumerate(prompts)]
    _compare("f16", cfg, grouped, singles)
    return plan


def test_fp16_nf4_grouped(dev):
    plan = _quantised_case(dev, load_in_4bit=True)
    assert plan["shared"] is True and plan["encoder_frames"] == 1 and plan["shared_prefix_ids"] == 4


def test_int8_takes_the_fallback(dev):
    plan = _quantised_case(dev, load_in_8bit=True)
    assert plan["shared"] is False and plan["encoder_frames"] == 1 and plan["shared_prefix_ids"] == 0


def test_graph_decode_replay_gives_the_first_calls_bits(dev):
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip = _setup("bf16", 1)
    model = LisaMI355(cfg, sd, dtype=torch.bfloat16, device=dev)
    assert model.decode_graphs is True
    S = cfg.sam.img_size
    ids, mask = _pad(cfg, _prompts(cfg, (3, 9)))
    forced = _forced(cfg)[[0, 2]]
    sizes = [(S, S)]
    run = lambda: model.evaluate(images_clip.to(dev), images.to(dev), ids.to(dev), sizes, sizes, max_new_tokens=5,   # noqa: E731
                                 forced_answer=forced, attention_mask=mask, offset=torch.tensor([0, 2]))
    first = run()
    assert model.last_group_plan["shared"] is True
    assert any(k[0] == "book" for k in model._graphs)      # the decode step of this shape was captured ...
    n_graphs = len(model._graphs)
    second = run()                                         # ... and is replayed here
    assert len(model._graphs) == n_graphs
    _bits_equal(first, second)
    model.decode_graphs = False
    eager = run()
    assert torch.equal(eager[0], first[0])


def _robot_request(inp, lines, rng_seed=12):
    from PIL import Image
    rng = np.random.default_rng(rng_seed)
    inp.mkdir()
    H, W = 150, 224
    Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(inp / "img.png")
    (inp / "prompt.txt").write_text("".join(line + "\n" for line in lines))
    (inp / "margins.txt").write_text("3,-2,5,1\n")
    for s in ("left", "right"):
        Image.fromarray(rng.integers(0, 256, (H - 1, W + 8), dtype=np.uint8)).save(inp / f"mask_{s}.png")


@pytest.mark.timeout(600)
def test_robot_demo_multi_prompt(dev, tmp_path, monkeypatch):
    from haff import lisa, robot_demo
    lines = ["open the drawer", "close the drawer", "pick up the cup by its handle"]
    orig = lisa.LisaMI355.evaluate
    calls = []

    def forced(self, *a, **kw):   # random-init models never emit [SEG]: force one so the mask branch runs
        n = a[2].shape[0]
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(n, -1).contiguous()
        kw["max_new_tokens"] = 3
        calls.append((n, kw.get("offset")))
        res = orig(self, *a, **kw)
        calls.append(dict(self.last_group_plan))
        return res
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", forced)
    flags = ["--synthetic", "tiny", "--force_left", "--image_size", "224", "--poll-interval", "0"]

    def run(name, lines, multi):
        inp, out = tmp_path / (name + "_in"), tmp_path / (name + "_out")
        _robot_request(inp, lines)
        robot_demo.main(flags + ["--zed2_img_path", str(inp), "--vis_save_path", str(out)] + (["--multi_prompt"] if multi else []),
                        max_requests=1)
        assert sorted(os.listdir(inp)) == ["mask_left.png", "mask_right.png"]
        return out
    names = ("aff_left", "aff_left_heat", "cropped_img")
    multi = run("multi", lines, True)
    assert calls[0][0] == 3 and calls[0][1].tolist() == [0, 3]
    assert calls[1]["shared"] is True and calls[1]["encoder_frames"] == 1 and calls[1]["rows"] == 3
    want = sorted(f"{n}{s}.png" for n in names for s in ("", "_1", "_2"))
    assert sorted(os.listdir(multi)) == want               # all nine outputs
    first = run("first", lines[:1], False)
    assert sorted(os.listdir(first)) == sorted(f"{n}.png" for n in names)
    third = run("third", lines[2:], False)
    for n in names:
        assert (multi / f"{n}.png").read_bytes() == (first / f"{n}.png").read_bytes(), n          # line 0: byte-equal
        assert (multi / f"{n}_2.png").read_bytes() == (third / f"{n}.png").read_bytes(), n        # line 2 == a one-line run of it
    assert (multi / "aff_left_1.png").read_bytes() != (multi / "aff_left_heat_1.png").read_bytes()
    sys.stdout.flush()
