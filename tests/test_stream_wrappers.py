"""tests/side_stream.py's registry against the package, without a GPU: every
public callable of lsbm_amd with a `stream` parameter has an entry, no entry
names something that is gone, and every entry's expected answer can tell a
zero-fill that lands after the kernel from a correct run.
"""
import importlib
import inspect
import os
import pkgutil
import re

import pytest

import side_stream as ss

# callables with a `stream` parameter that need no entry: helpers behind the
# public ones, which pass the stream through
EXEMPT = {
    "engine._stream_ptr": "turns a stream (None: torch's current one) into the void* the C ABI takes",
    "scan.SnapshotView._end": "the body of seek_to_first / seek_to_last, which have entries",
}


def stream_callables():
    """{name: callable} of every function of an lsbm_amd module, and every
    method of a class defined there, whose signature has `stream`."""
    import lsbm_amd
    found = {}
    for info in pkgutil.iter_modules(lsbm_amd.__path__):
        if not os.path.exists(os.path.join(lsbm_amd.__path__[0], info.name + ".py")):
            continue  # (the product library lies beside the modules)
        mod = importlib.import_module("lsbm_amd." + info.name)
        for name, obj in vars(mod).items():
            if getattr(obj, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(obj):
                if "stream" in inspect.signature(obj).parameters:
                    found[f"{info.name}.{name}"] = obj
            elif inspect.isclass(obj):
                for attr, member in vars(obj).items():
                    member = getattr(member, "__func__", member)
                    if inspect.isfunction(member) and "stream" in inspect.signature(member).parameters:
                        found[f"{info.name}.{name}.{attr}"] = member
    return found


def test_every_stream_taking_callable_is_registered():
    found = stream_callables()
    assert len(found) == 97
    assert all(name.rsplit(".", 1)[1].startswith("_") for name in EXEMPT), "only underscore helpers are exempt"
    assert all(reason for reason in EXEMPT.values())
    assert not set(EXEMPT) & set(ss.REGISTRY)
    missing = sorted(set(found) - set(ss.REGISTRY) - set(EXEMPT))
    assert not missing, missing
    gone = sorted((set(ss.REGISTRY) | set(EXEMPT)) - set(found))
    assert not gone, gone


def test_every_public_one_is_wrapped_in_on_stream():
    """engine.on_stream is what puts a call's allocations, fills, torch glue,
    launches and host reads on its `stream`: no public callable goes without."""
    for name, fn in stream_callables().items():
        if name not in EXEMPT:
            assert hasattr(fn, "__wrapped__") and "stream" in inspect.signature(fn.__wrapped__).parameters, name


@pytest.mark.parametrize("name", sorted(ss.REGISTRY))
def test_expected_answer_is_not_all_zeros(name):
    e = ss.REGISTRY[name]
    want = e.want()
    assert isinstance(want, dict) and want
    assert any(ss.nonzero(v) for v in want.values()), "a late zero-fill would pass for a correct run"
    assert set(e.own) <= set(want), sorted(set(e.own) - set(want))
    if e.own:
        assert e.creates_nothing is None
        assert any(ss.nonzero(want[k]) for k in e.own), "no output that the wrapper creates itself is non-zero"
    else:
        assert e.creates_nothing, "an entry without an output of the wrapper's own says why"


def test_the_stream_is_the_trailing_argument_of_every_dev_function():
    """What the GPU tests' spy reads as the stream: the last parameter of every
    *_dev declaration of include/*.h is `void* stream`, and _lib.py's tables
    have as many arguments as the declaration has parameters."""
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    declared = {}
    for name in sorted(os.listdir(include)):
        if name.endswith(".h"):
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, name)).read(), flags=re.S)
            for fn, params in re.findall(r"\b(lsbm_\w+_dev)\s*\(([^;{]*)\)\s*;", text):
                declared[fn] = [p.strip() for p in params.split(",")]
    at = ss.stream_positions()
    assert set(at) == set(declared) and len(at) >= 60
    for fn, params in declared.items():
        assert re.fullmatch(r"void\s*\*\s*stream", params[-1]), (fn, params[-1])
        assert at[fn] == len(params) - 1, fn
