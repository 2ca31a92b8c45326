"""prompt_groups: the host bookkeeping of LisaMI355.evaluate(offset=) — which frame a prompt row belongs to and how many leading ids
the rows of a call can share. Pure integer work on the CPU: the module must import without the HIP library."""
import subprocess
import sys

import pytest
import torch

from haff import prompt_groups as G

SEG = 900
HEAD = [1, 901, -200, 902, 13, 77]          # bos, <im_start>, <image>, <im_end>, two words of the question


def _rows(rows, pad=0):
    L = max(len(r) for r in rows)
    ids = torch.full((len(rows), L), pad, dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
    return ids, torch.tensor([len(r) for r in rows])


def test_identical_heads_share_the_head():
    ids, lens = _rows([HEAD + [5, 6, 7], HEAD + list(range(20, 29)), HEAD + list(range(40, 46))])
    assert G.shared_prefix_len(ids, lens, SEG) == len(HEAD)
    assert G.prefix_positions(len(HEAD), 256) == len(HEAD) + 255 and G.prefix_positions(0, 256) == 0


def test_tails_that_start_alike_extend_the_prefix():
    ids, lens = _rows([HEAD + [5, 6, 7], HEAD + [5, 6, 9, 9]])
    assert G.shared_prefix_len(ids, lens, SEG) == len(HEAD) + 2


def test_a_row_that_is_a_prefix_of_another_keeps_one_id_of_its_own():
    short = HEAD + [5, 6]
    ids, lens = _rows([short, short + [7, 8, 9]])
    assert G.shared_prefix_len(ids, lens, SEG) == len(short) - 1
    # ... also when the padding id happens to continue the match
    ids, lens = _rows([short, short + [0, 0]], pad=0)
    assert G.shared_prefix_len(ids, lens, SEG) == len(short) - 1


def test_seg_in_the_common_head_cuts_in_front_of_the_id_it_reads():
    head = HEAD + [SEG, 14]                  # [SEG] at id position 6 reads the hidden state of id position 5
    ids, lens = _rows([head + [5, 6, 7], head + [8, 9]])
    assert G.shared_prefix_len(ids, lens, SEG) == 5
    # a [SEG] in ONE row's own tail right behind the head: the head's last id stays with the rows
    ids, lens = _rows([HEAD + [SEG, 7], HEAD + [8, 9, 10]])
    assert G.shared_prefix_len(ids, lens, SEG) == len(HEAD) - 1
    # a pad id equal to [SEG] behind a row's end is no [SEG]
    ids, lens = _rows([HEAD + [5, 6, 7], HEAD + [8]], pad=SEG)
    assert G.shared_prefix_len(ids, lens, SEG) == len(HEAD)


def test_rows_that_differ_before_the_sentinel_share_nothing():
    ids, lens = _rows([[1, 901, -200, 902, 5, 6], [1, 903, -200, 902, 5, 6]])
    assert G.shared_prefix_len(ids, lens, SEG) == 0
    # identical up to but not past the sentinel: nothing worth sharing either
    ids, lens = _rows([[1, 901, -200, 902], [1, 901, 7, -200]])
    assert G.shared_prefix_len(ids, lens, SEG) == 0
    # [SEG] so early that the cut falls on the sentinel
    ids, lens = _rows([[1, -200, 5, SEG, 8], [1, -200, 5, SEG, 9]])
    assert G.shared_prefix_len(ids, lens, SEG) == 2
    ids, lens = _rows([[1, -200, SEG, 8], [1, -200, SEG, 9]])
    assert G.shared_prefix_len(ids, lens, SEG) == 0


def test_single_row():
    ids, lens = _rows([HEAD + [5, 6, 7]])
    P = G.shared_prefix_len(ids, lens, SEG)
    assert 0 < P <= ids.shape[1] - 1


def test_check_offset_accepts():
    assert G.check_offset(torch.tensor([0, 3, 5]), 5, 2).tolist() == [0, 0, 0, 1, 1]
    assert G.check_offset(torch.tensor([0, 0, 2]), 2, 2).tolist() == [1, 1]                   # an empty frame
    assert G.check_offset(torch.tensor([0, 2, 2, 3]), 3, 3).tolist() == [0, 0, 2]             # an empty middle frame
    f = G.check_offset(torch.arange(5), 4, 4)
    assert f.tolist() == [0, 1, 2, 3] and f.dtype == torch.int32 and f.device.type == "cpu"
    assert G.check_offset([0, 3], 3, 1).tolist() == [0, 0, 0]                                 # a list of ints is taken as int64
    assert G.is_identity(torch.arange(5)) and G.is_identity([0, 1]) and not G.is_identity(torch.tensor([0, 2])) \
        and not G.is_identity(torch.tensor([0, 0, 2]))


@pytest.mark.parametrize("offset,B,F", [
    (torch.tensor([0, 3, 2, 5]), 5, 3),                       # decreasing
    (torch.tensor([0, 3, 4]), 5, 2),                          # last value is not B
    (torch.tensor([0, 3, 5], dtype=torch.int32), 5, 2),       # dtype
    (torch.tensor([0.0, 3.0, 5.0]), 5, 2),                    # dtype
    (torch.tensor([0, 3, 5]), 5, 3),                          # length is not F + 1
    (torch.tensor([[0, 3, 5]]), 5, 2),                        # not one-dimensional
    (torch.tensor([1, 3, 5]), 5, 2),                          # does not start at 0
    ([0, 2.5, 5], 5, 2),                                      # a list that is not ints
])
def test_check_offset_rejects_and_names_the_argument(offset, B, F):
    with pytest.raises(ValueError, match="offset"):
        G.check_offset(offset, B, F)


def test_module_imports_without_the_library():
    """The bookkeeping is importable where there is no HIP library at all: importing it loads neither haff.lib's library nor haff.ops."""
    code = ("import sys, haff\nfrom haff import prompt_groups, lib\n"
            "assert lib._lib is None and 'haff.ops' not in sys.modules and '2handedafforder_amd.ops' not in sys.modules\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
