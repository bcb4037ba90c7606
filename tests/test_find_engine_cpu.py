"""CPU: verify-and-find has one host engine (csrc/find.hpp: FindEngine) under its three modes -- rewinding, rewinding with
view tags, per output (csrc/outputs.hpp supplies that class step) -- and one entry shim in capi.hip.  Read from the sources:
the copies that the per-output call was first written as are gone, and what the engine says once is said once."""

import re

from test_abi_guard_cpu import _csrc_sources


def _count(needle, *texts):
    return sum(t.count(needle) for t in texts)


def test_find_calls_share_one_engine_and_one_shim():
    src = _csrc_sources()
    assert len(src) > 40 and {"capi.hip", "find.hpp", "outputs.hpp"} <= set(src)
    # the second argument struct, the adapter that fed it to find_nothing and the second pair bound are gone
    for name in ("OutputsArgs", "counts_only", "out_pairs_bounded"):
        assert not [f for f, text in src.items() if re.search(r"\b%s\b" % name, text)], name
    # one text for an m_i no engine takes, whoever asks
    assert _count('": not a power of two"', *src.values()) == 1 and '": not a power of two"' in src["scan_args.hpp"]
    # one compaction and one front
    assert _count("hipLaunchKernelGGL(k_find_emit<", *src.values()) == 1
    assert _count("V::decode_front(", src["find.hpp"], src["outputs.hpp"]) == 1
    # the engine, its host twin included, is in find.hpp; outputs.hpp instantiates it and defines neither again
    assert "struct FindEngine" in src["find.hpp"] and "FindEngine<C, OutputStep<C>>" in src["outputs.hpp"]
    assert _count("BlockUpload up;", src["find.hpp"], src["outputs.hpp"]) == 1
    assert "struct Layout" not in src["outputs.hpp"]
