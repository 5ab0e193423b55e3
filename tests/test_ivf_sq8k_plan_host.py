"""The plugin parameter `direct_kloop` (option "ivf_sq8_kloop", csrc/ivf_sq8d_plan.hpp) against the fake library of the plugin contract
tests: it reaches vdb_set_option, and before the rows are added.  No GPU.  (The chunk and K-order rules of the scan are exercised by
tests/test_gpu_ivf_sq8_kloop.py at D = 132 / 200 / 1000.)"""
from __future__ import annotations

import pytest

from tests.test_plugin_contract_host import DIM, H, X, fake  # noqa: F401


@pytest.mark.parametrize("value", [True, False])
def test_direct_kloop_of_the_plugin_classes_reaches_set_option_before_the_add(fake, value):  # noqa: F811
    import vdbhip.ivf as ivf

    want = [(H, b"ivf_sq8_kloop", float(value))]

    def set_before_add():
        names = fake.names()
        return fake.calls("vdb_set_option") == want and names.index("vdb_set_option") < min(i for i, n in enumerate(names) if n.startswith("vdb_ivf_add"))

    art = ivf.HipIVFIndexer("ix", DIM, "l2", index_key="IVF4,SQ8", direct_kloop=value).build(X)
    assert set_before_add(), fake.names()
    fake.clear()
    s = ivf.HipIVFSearcher("s", DIM, "l2", direct_kloop=value)
    s.attach(art, X)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    ivf.HipApproximateSearch("a", DIM, "IVF4,SQ8", "l2", direct_kloop=value).build_index(X)
    assert set_before_add(), fake.names()
    fake.clear()
    ivf.IVFSQ8Index(DIM, 4, "l2", 0, direct_kloop=value)
    assert fake.calls("vdb_set_option") == want
    fake.clear()
    ivf.HipIVFIndexer("ix", DIM, "l2", index_key="IVF4,SQ8").build(X)          # not given: the option is never touched
    assert fake.calls("vdb_set_option") == []
