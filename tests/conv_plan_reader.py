"""Work plans of the training convolutions as the launchers compute them: ``tests/conv_plan_tool.cpp`` in print mode, which includes
``csrc/conv3d_plan.h`` and ``csrc/bf16_conv_plan.h`` - the headers the launchers launch from.  The tool is built once per session (host
code only) into a temporary directory; child processes find it through ``MVS_CONV_PLAN_TOOL``.  No GPU code."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

_ENV = "MVS_CONV_PLAN_TOOL"
_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plan_tool.cpp")
_TEXT_FIELDS = ("form", "route")          # "22" and "42" are names, not numbers


def tool():
    """Path of the built tool."""
    exe = os.environ.get(_ENV)
    if exe and os.path.exists(exe):
        return exe
    tmp = tempfile.mkdtemp(prefix="conv_plan_tool_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "conv_plan_tool")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-x", "hip", "--offload-host-only", _SRC, "-o", exe])
    os.environ[_ENV] = exe
    return exe


def _value(name, text):
    if name in _TEXT_FIELDS:
        return text
    if text in ("true", "false"):
        return text == "true"
    if "," in text:
        return tuple(int(v) for v in text.split(","))
    return int(text)


@functools.lru_cache(maxsize=None)
def fields(kind, *args):
    """One request -> dict of the fields the tool prints for it."""
    request = " ".join([kind] + [str(int(a)) if isinstance(a, bool) else str(a) for a in args])
    out = subprocess.run([tool(), "print"], input=request + "\n", capture_output=True, text=True, check=True).stdout.split()
    got = dict(item.split("=", 1) for item in out)
    assert got and "error" not in got, (request, out)
    return {k: _value(k, v) for k, v in got.items()}


def plan(ntuple, kind, *args, **derived):
    """The named tuple ``ntuple`` from the tool's fields of that name (+ ``derived`` ones the caller computes from them)."""
    got = dict(fields(kind, *args), **derived)
    return ntuple(*(got[f] for f in ntuple._fields))
