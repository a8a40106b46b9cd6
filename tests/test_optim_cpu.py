"""CPU suite for the optimizer step (include/hsr_optim.h, hsr_utils/optim.py): the table entry's layout agrees with the library,
host-side argument checks work without a GPU, and on CPU tensors hsr_utils.optim.Adam is torch.optim.Adam (every tensor falls back to
torch's own functional adam()).  The header's prototypes are exported and bound with the right types (the one checker of tests/test_abi.py)."""
import ctypes as C
import os
import re

import torch

from test_abi import check_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsr_optim.h")


def test_header_prototypes_are_exported_and_bound():
    assert check_header("hsr_optim.h") == ["hsr_adam_table_entry_bytes", "hsr_adam_step", "hsr_track_keep_best"]


def test_table_entry_layout_matches_the_library():
    from hsr_utils import optim
    assert optim._lib.hsr_adam_table_entry_bytes() == C.sizeof(optim._AdamTensor) == 64
    src = open(HEADER).read()
    fields = re.search(r"typedef struct hsr_adam_tensor \{(.*?)\} hsr_adam_tensor;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [f[0] for f in optim._AdamTensor._fields_]
    assert int(re.search(r"#define HSR_ADAM_MAX_TENSORS (\d+)", src).group(1)) == 32


def test_argument_errors_without_gpu():
    from hsr_utils import optim
    lib = optim._lib
    assert lib.hsr_adam_step(-1, None, None) < 0 and b"adam_step" in lib.hsr_last_error()
    assert lib.hsr_adam_step(1, None, None) < 0
    assert lib.hsr_adam_step(0, None, None) == 0       # an empty table is a no-op
    bad = (optim._AdamTensor * 1)()
    bad[0].numel = 5                                   # NULL pointers with numel > 0
    assert lib.hsr_adam_step(1, bad, None) < 0 and b"entry 0" in lib.hsr_last_error()
    bad[0].numel = -1
    assert lib.hsr_adam_step(1, bad, None) < 0
    assert lib.hsr_track_keep_best(0, 0, *([None] * 6), None) < 0 and b"track_keep_best" in lib.hsr_last_error()
    assert lib.hsr_track_keep_best(4, 4, *([None] * 6), None) < 0


def _model(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((7,), (5, 3), (1,), (0, 4))]


def _grads(params, it):
    g = torch.Generator().manual_seed(100 + it)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * (10.0 ** (it % 5 - 2))


def test_cpu_tensors_fall_back_to_torch_bit_for_bit():
    from hsr_utils.optim import Adam
    a, b = _model(0), _model(0)
    groups = lambda ps: [{"params": ps[:2], "lr": 1e-2}, {"params": ps[2:], "lr": 0.0, "eps": 1e-15}]
    oa, ob = Adam(groups(a), betas=(0.8, 0.99)), torch.optim.Adam(groups(b), betas=(0.8, 0.99))
    for it in range(6):
        _grads(a, it); _grads(b, it)
        if it == 2:                                    # a grad of None: no state, no step
            a[1].grad = b[1].grad = None
        oa.step(); ob.step()
        assert oa.last_fused_tensors == 0
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for k in sb["state"]:
        for n in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][k][n], sb["state"][k][n]), (k, n)
    # state_dict round trip torch -> hsr and hsr -> torch, then training continues identically
    c, d = [p.detach().clone().requires_grad_(True) for p in a], [p.detach().clone().requires_grad_(True) for p in b]
    oc, od = torch.optim.Adam(groups(c)), Adam(groups(d))
    oc.load_state_dict(sa); od.load_state_dict(sb)
    assert od.state_dict()["state"][0]["step"].dtype == torch.float32 and not od.state_dict()["state"][0]["step"].is_cuda
    for it in range(6, 9):
        _grads(c, it); _grads(d, it)
        oc.step(); od.step()
        for x, y in zip(c, d):
            assert torch.equal(x, y)
