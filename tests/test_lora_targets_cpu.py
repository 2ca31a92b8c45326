"""--lora_target_modules on the host: the reference's target rule (find_linear_layers, train_ds.py:195-214) over the seven Llama
projections, its errors, the adapter shapes, counts and peft initialisation, and the resume check on mismatched adapters."""
import math
from types import SimpleNamespace

import pytest
import torch

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"


def _mods():
    import haff  # noqa: F401
    from haff import config as hcfg, train_model as TM
    return hcfg, TM


def test_spec_to_module_set():
    hcfg, TM = _mods()
    cfg = hcfg.tiny()   # 2 layers
    assert TM.lora_targets(cfg, "q_proj,v_proj") == ["model.layers.0.self_attn.q_proj", "model.layers.0.self_attn.v_proj",
                                                      "model.layers.1.self_attn.q_proj", "model.layers.1.self_attn.v_proj"]
    every = TM.lora_targets(cfg, "proj")
    assert every == TM.lora_targets(cfg, ALL7) == TM.lora_targets(cfg, ALL7.split(","))
    assert every[:7] == ["model.layers.0.self_attn.q_proj", "model.layers.0.self_attn.k_proj", "model.layers.0.self_attn.v_proj",
                         "model.layers.0.self_attn.o_proj", "model.layers.0.mlp.gate_proj", "model.layers.0.mlp.up_proj",
                         "model.layers.0.mlp.down_proj"]
    assert len(every) == 14
    assert TM.lora_targets(cfg, "mlp") == [m for m in every if ".mlp." in m]
    assert TM.lora_targets(cfg, "layers.1.self_attn.o_proj") == ["model.layers.1.self_attn.o_proj"]
    assert TM.lora_targets(cfg, " up_proj , gate_proj") == [m for m in every if m.endswith(("gate_proj", "up_proj"))]


def test_spec_errors():
    hcfg, TM = _mods()
    cfg = hcfg.tiny()
    with pytest.raises(ValueError, match="not found"):
        TM.lora_targets(cfg, "q_proj,qq_proj")
    with pytest.raises(ValueError, match="lm_head"):
        TM.lora_targets(cfg, "q_proj,lm_head")
    with pytest.raises(ValueError, match="lm_head"):
        TM.lora_targets(cfg, "head")
    with pytest.raises(ValueError, match="not found"):   # skipped by the rule, as the reference's
        TM.lora_targets(cfg, "text_hidden_fcs")


def test_7b_parameter_counts_and_shapes():
    hcfg, TM = _mods()
    cfg = hcfg.haff_7b()
    assert (cfg.llm.hidden, cfg.llm.layers, cfg.llm.ffn) == (4096, 32, 11008)
    shapes = {"q_proj": (4096, 4096), "k_proj": (4096, 4096), "v_proj": (4096, 4096), "o_proj": (4096, 4096),
              "gate_proj": (4096, 11008), "up_proj": (4096, 11008), "down_proj": (11008, 4096)}

    def count(spec, r=8):
        return sum(r * shapes[m.rsplit(".", 1)[1]][0] + shapes[m.rsplit(".", 1)[1]][1] * r for m in TM.lora_targets(cfg, spec))
    assert count("q_proj,v_proj") == 4_194_304
    assert count(ALL7) == 19_988_480
    small = hcfg.tiny()
    sd = TM.init_lora(small, TM.lora_targets(small, ALL7), 8, seed=0)
    H, F = small.llm.hidden, small.llm.ffn
    assert sd["model.layers.1.mlp.down_proj.lora_A"].shape == (8, F) and sd["model.layers.1.mlp.down_proj.lora_B"].shape == (H, 8)
    assert sd["model.layers.0.mlp.gate_proj.lora_A"].shape == (8, H) and sd["model.layers.0.mlp.gate_proj.lora_B"].shape == (F, 8)
    assert sum(t.numel() for t in sd.values()) == 2 * (4 * 16 * H + 3 * 8 * (H + F))


def test_init_matches_peft_and_default_is_bit_identical():
    hcfg, TM = _mods()
    cfg = hcfg.mid()
    H, F = cfg.llm.hidden, cfg.llm.ffn
    # what LisaTrainable drew before targets were configurable: q, v of every layer from one generator, bound 1/sqrt(H)
    g = torch.Generator(device="cpu").manual_seed(7)
    old = {}
    for i in range(cfg.llm.layers):
        for n in ("q_proj", "v_proj"):
            k = f"model.layers.{i}.self_attn.{n}"
            old[k + ".lora_A"] = (torch.rand((8, H), generator=g) * 2 - 1) * (1.0 / math.sqrt(H))
            old[k + ".lora_B"] = torch.zeros((H, 8))
    new = TM.init_lora(cfg, TM.lora_targets(cfg, "q_proj,v_proj"), 8, seed=7)
    assert list(new) == list(old)
    for k in old:
        assert torch.equal(new[k], old[k]), k
    allp = TM.init_lora(cfg, TM.lora_targets(cfg, ALL7), 8, seed=7)
    for k, t in allp.items():
        if k.endswith("lora_B"):
            assert not t.any()
        else:
            fan_in = t.shape[1]
            assert fan_in == (F if "down_proj" in k else H)
            assert t.abs().max() <= 1.0 / math.sqrt(fan_in) and t.abs().max() > 0.9 / math.sqrt(fan_in), k
    # the draw order: layer by layer, q k v o gate up down; an unselected module draws nothing
    qk = TM.init_lora(cfg, TM.lora_targets(cfg, "q_proj,k_proj"), 8, seed=7)
    assert torch.equal(qk["model.layers.0.self_attn.q_proj.lora_A"], allp["model.layers.0.self_attn.q_proj.lora_A"])
    assert torch.equal(qk["model.layers.0.self_attn.k_proj.lora_A"], allp["model.layers.0.self_attn.k_proj.lora_A"])
    assert not torch.equal(qk["model.layers.1.self_attn.q_proj.lora_A"], allp["model.layers.1.self_attn.q_proj.lora_A"])


def test_resume_with_other_targets_names_the_keys():
    hcfg, TM = _mods()
    cfg = hcfg.tiny()
    mine = TM.init_lora(cfg, TM.lora_targets(cfg, "q_proj,v_proj"), 8)
    ckpt = TM.init_lora(cfg, TM.lora_targets(cfg, ALL7), 8)
    fake = SimpleNamespace(params=dict(mine), lora_modules=TM.lora_targets(cfg, "q_proj,v_proj"))
    with pytest.raises(ValueError, match=r"extra keys \['model.layers.0.mlp.down_proj.lora_A'") as e:
        TM.LisaTrainable.load_state_dict(fake, ckpt)
    assert "(20)" in str(e.value) and "missing keys [] (0)" in str(e.value)
    fake = SimpleNamespace(params=dict(ckpt), lora_modules=TM.lora_targets(cfg, ALL7))
    with pytest.raises(ValueError, match=r"missing keys \['model.layers.0.mlp.down_proj.lora_A'"):
        TM.LisaTrainable.load_state_dict(fake, mine)
    TM.LisaTrainable.load_state_dict(SimpleNamespace(params={k: v.clone() for k, v in mine.items()}, lora_modules=[]), mine)
