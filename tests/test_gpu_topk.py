"""The wave top-k (csrc/topk.hpp) on its own: synthetic partial lists through both merge entry points against the C oracle.

merge_kernel feeds element i = p * k + j of the concatenated parts, 64 at a time, into WaveTopK<kpl_for(k)>::offer, so the
entry points are the select as a pure function of keys and ids in device memory.  The cases (tests/topk_cases.py) cover
k = 1 ... 2048 on both sides of every list-width boundary, both metrics, ties, short and empty lists, extreme key values and
launch shapes; tests/test_topk_host.py proves on the host that each branch case reaches the serial route into a full list
(register-crossing shifts included), the batch merge into a full and into a partly filled list, and offers of exactly 11,
12 and 13 accepted pairs.

Mixed signed zeros in one list are outside the contract: `sortable_u64` orders -0.0 below +0.0 and the oracle's double
comparison does not.  The kernels produce +0.0 under l2 and -0.0 under ip only, and so do the cases; none feeds both.
Comparisons are exact: np.testing.assert_array_equal on ids and float32 distances.
"""
from __future__ import annotations

import numpy as np
import pytest

from . import topk_cases as tc

pytestmark = pytest.mark.gpu


def _merge_both(vdb, c):
    """(D, I) of vdb_merge_partials_device and of the packed form, given the same data."""
    import torch

    dev = torch.device("cuda", 0)
    nparts, nq, k = c.keys.shape
    keys = torch.from_numpy(c.keys).to(dev)
    ids = torch.from_numpy(c.ids).to(dev)
    out = []
    for packed in (False, True):
        D = torch.full((nq, k), 123.0, dtype=torch.float32, device=dev)
        I = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
        if packed:
            pack = torch.stack([keys.view(torch.int64), ids], dim=1).contiguous()      # (nparts, 2, nq, k)
            vdb.merge_packed_partials_device(c.metric, 0, pack.data_ptr(), nparts, nq, k, D.data_ptr(), I.data_ptr())
        else:
            vdb.merge_partials_device(c.metric, 0, keys.data_ptr(), ids.data_ptr(), nparts, nq, k, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        out.append((D.cpu().numpy(), I.cpu().numpy()))
    return out


@pytest.mark.parametrize("name", tc.case_names())
def test_merge_case(vdb, oracle, name):
    c = tc.case_by_name(name)
    Do, Io = oracle.merge_partials(c.keys, c.ids, c.metric)
    for form, (D, I) in zip(("split", "packed"), _merge_both(vdb, c)):
        np.testing.assert_array_equal(I, Io, err_msg=f"{name} ({form})")
        np.testing.assert_array_equal(D, Do, err_msg=f"{name} ({form})")
