"""The wave votes' counters (option vote_stats, wost_device.h WOST_VOTE) exist only in
the study build: the product library's generated kernels are the same bytes with the
tool's variable set, and carry no counter."""
import test_options as TO


def test_product_kernels_ignore_the_vote_stats_variable():
    base = TO._sources({})
    ab = TO._sources({"WOST_VOTE_STATS": "1"})
    assert ab["report"] == {"build": "product", "non_default": {}}
    for name in ("dcr_dipole", "wenner_topography", "variable_coefficients"):
        assert ab[name] == base[name], name
        assert "WOST_VOTE" not in ab[name]
