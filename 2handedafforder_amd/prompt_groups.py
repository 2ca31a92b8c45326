"""Bookkeeping of LisaMI355.evaluate(offset=): several prompt rows on one frame, the reference's `model_forward(..., offset, ...)`
convention (LISA.py:224-262: conversations offset[i]:offset[i+1] belong to image i). Host arithmetic on small integer tensors only:
nothing here loads the HIP library or touches a device.
"""
import torch

IMAGE_TOKEN_INDEX = -200


def check_offset(offset, B, F):
    """offset (int64 [F+1]: offset[0] == 0, non-decreasing, offset[-1] == B; a list of ints is taken as one) -> frame_of int32 [B] on
    the CPU: row b belongs to frame f where offset[f] <= b < offset[f+1]. A frame may have no rows. Anything else is a ValueError
    that names the argument."""
    if isinstance(offset, (list, tuple)):
        if not all(isinstance(o, int) and not isinstance(o, bool) for o in offset):
            raise ValueError(f"offset: a list of ints or an int64 tensor is expected, got {offset!r}")
        offset = torch.tensor(list(offset), dtype=torch.int64)
    if not isinstance(offset, torch.Tensor) or offset.dtype != torch.int64:
        raise ValueError(f"offset: an int64 tensor [F+1] is expected, got {getattr(offset, 'dtype', type(offset).__name__)}")
    if offset.dim() != 1 or offset.numel() != F + 1:
        raise ValueError(f"offset: {F} frames need F+1 = {F + 1} entries, got shape {tuple(offset.shape)}")
    off = offset.tolist()            # F + 1 python ints: the checks below cost the plain path (one row per frame) a few microseconds
    if off[0] != 0:
        raise ValueError(f"offset: offset[0] must be 0, got {off[0]}")
    if any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"offset: must be non-decreasing, got {off}")
    if off[-1] != B:
        raise ValueError(f"offset: offset[-1] must be the number of prompt rows ({B}), got {off[-1]}")
    return torch.tensor([f for f in range(F) for _ in range(off[f + 1] - off[f])], dtype=torch.int32)


def is_identity(offset):
    """offset (as accepted by check_offset) is arange(F+1): one row per frame, the plain evaluate() call."""
    off = offset.tolist() if isinstance(offset, torch.Tensor) else list(offset)
    return off == list(range(len(off)))


def shared_prefix_len(input_ids, lens, seg_token_idx):
    """The id-prefix length P that every row of input_ids [B, L] (right-padded; lens [B] real ids per row) can share: the longest
    run of leading columns that is identical in ALL rows, cut so that
      (i)   it contains the <image> sentinel (else there is nothing worth sharing: 0);
      (ii)  it ends before the id in FRONT of the first [SEG] of any row: [SEG] at id position s makes seg_embeddings read the hidden
            state of id position s - 1 (LISA.py:457-465), and the shared part's hidden rows are never produced, so P <= s - 1;
      (iii) P <= min(lens) - 1: every row keeps at least one id of its own (its last real position yields the first token).
    Returns 0 when no such prefix holds the sentinel."""
    ids = input_ids.detach().cpu()
    lens = torch.as_tensor(lens).detach().cpu().long()
    B, L = ids.shape
    if B == 0 or L == 0:
        return 0
    differs = (ids != ids[:1]).any(0)
    P = int(differs.int().argmax()) if bool(differs.any()) else L
    P = min(P, int(lens.min()) - 1)
    real = torch.arange(L)[None, :] < lens[:, None]
    seg = ((ids == seg_token_idx) & real).any(0)
    if bool(seg.any()):
        P = min(P, int(seg.int().argmax()) - 1)
    if P <= 0:
        return 0
    sentinel = (ids[0, :P] == IMAGE_TOKEN_INDEX).nonzero()
    return P if sentinel.numel() > 0 else 0


def prefix_positions(P, n_img):
    """Cache positions of a P-id prefix once the sentinel is replaced by its n_img image rows."""
    return P + n_img - 1 if P > 0 else 0
