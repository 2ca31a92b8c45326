"""fp16 fine-tuning, host side: the dynamic loss scaler (a restatement of DeepSpeed's fp16 defaults: the reference's engine config
enables fp16 and states nothing else, train_ds.py:365-370) against hand-computed sequences, and train_ds's --precision mapping."""
import pytest
import torch

from haff import train_ops as T
from haff import train_ds


def test_defaults_are_deepspeeds():
    s = T.DynamicLossScaler()
    assert s.loss_scale == 2.0 ** 16
    assert (s.scale_factor, s.scale_window, s.delayed_shift, s.min_scale) == (2.0, 1000, 2, 1.0)
    assert not s.consecutive_hysteresis and s.raise_error_at_min_scale


def test_single_overflow_spends_hysteresis_and_keeps_the_scale():
    s = T.DynamicLossScaler()
    assert s.update_scale(True) is True
    assert s.loss_scale == 2.0 ** 16 and s.cur_hysteresis == 1
    assert s.last_overflow_iter == 0 and s.cur_iter == 1 and s.skipped_steps == 1


def test_two_overflows_in_a_row_halve_the_scale():
    s = T.DynamicLossScaler()
    s.update_scale(True)
    s.update_scale(True)
    assert s.loss_scale == 2.0 ** 15
    assert s.cur_hysteresis == 1              # not reset by the halving: only a window of clean steps resets it
    s.update_scale(True)                      # hysteresis already spent: every further overflow halves
    assert s.loss_scale == 2.0 ** 14 and s.skipped_steps == 3


def test_overflow_then_clean_steps_do_not_reset_hysteresis_before_the_window():
    s = T.DynamicLossScaler()
    s.update_scale(True)
    for _ in range(10):
        assert s.update_scale(False) is False
    assert s.cur_hysteresis == 1 and s.loss_scale == 2.0 ** 16
    s.update_scale(True)                      # the second overflow of the window halves
    assert s.loss_scale == 2.0 ** 15


def test_window_of_clean_steps_doubles_the_scale():
    s = T.DynamicLossScaler()
    for i in range(999):
        s.update_scale(False)
    assert s.loss_scale == 2.0 ** 16          # (iter - last_overflow_iter) % 1000 == 0 first holds at iter 999
    s.update_scale(False)
    assert s.loss_scale == 2.0 ** 17 and s.cur_iter == 1000
    for i in range(1000):
        s.update_scale(False)
    assert s.loss_scale == 2.0 ** 18


def test_window_counts_from_the_last_overflow_and_resets_hysteresis():
    s = T.DynamicLossScaler()
    s.update_scale(True)                      # iter 0: overflow, hysteresis 2 -> 1
    for _ in range(999):
        s.update_scale(False)                 # iters 1..999
    assert s.loss_scale == 2.0 ** 16 and s.cur_hysteresis == 1
    s.update_scale(False)                     # iter 1000: 1000 - 0 == window
    assert s.loss_scale == 2.0 ** 17 and s.cur_hysteresis == 2


def test_overflow_at_the_minimum_scale_raises():
    s = T.DynamicLossScaler(init_scale=4.0)
    s.update_scale(True)                      # hysteresis
    s.update_scale(True)                      # 4 -> 2
    s.update_scale(True)                      # 2 -> 1
    assert s.loss_scale == 1.0
    with pytest.raises(RuntimeError, match="minimum loss scale"):
        s.update_scale(True)
    q = T.DynamicLossScaler(init_scale=2.0, raise_error_at_min_scale=False)
    for _ in range(4):
        q.update_scale(True)
    assert q.loss_scale == 1.0                # clamped at min_scale when not raising


def test_state_round_trips_through_a_checkpoint_dict(tmp_path):
    s = T.DynamicLossScaler()
    for ov in (True, False, False, True, True, False):
        s.update_scale(ov)
    path = tmp_path / "latest.pt"
    torch.save({"loss_scaler": s.state_dict()}, path)
    r = T.DynamicLossScaler()
    r.load_state_dict(torch.load(path, weights_only=False)["loss_scaler"])
    assert r.state_dict() == s.state_dict()
    assert (r.loss_scale, r.cur_hysteresis, r.last_overflow_iter, r.cur_iter, r.skipped_steps) == (2.0 ** 14, 1, 4, 6, 3)
    for ov in (False, True, False):
        assert r.update_scale(ov) == s.update_scale(ov)
    assert r.state_dict() == s.state_dict()


def test_precision_flag_maps_to_the_trainer_dtype():
    assert train_ds.precision_dtype("fp16") == torch.float16
    assert train_ds.precision_dtype("bf16") == torch.bfloat16
    assert train_ds.precision_dtype("fp32") == torch.float32
    assert train_ds.parse_args(["--precision", "fp16"]).precision == "fp16"


def test_bucket_optimizer_copy_codes():
    """The fused AdamW kernel's code of a parameter copy per bucket dtype (bf16 0, fp16 3; fp32 buckets alias the master)."""
    assert T._LP_DT == {torch.bfloat16: 0, torch.float16: 3}
