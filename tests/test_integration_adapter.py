"""INTEGRATION.md section 2 (the MNN Creator / Execution adapter a maintainer adds to the reference)
calls only what this repository's include/niti_hip.h declares.  (Type-checking the adapter needs
the reference's own headers -- Execution.hpp, CPUBackend.hpp, MNN_generated.h -- which are source
and are not kept here: a maintainer's compiler does that check where the adapter is added.)"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def adapter_source():
    s = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blk = s[s.index("## 2. Adapter"):]
    code = blk[blk.index("```cpp") + len("```cpp"):]
    return code[:code.index("```")]


def test_integration_adapter_uses_declared_entry_points():
    """Every niti_* call in the adapter is a function include/niti_hip.h declares."""
    import re

    from niti_amd import _lib
    declared = set(_lib.header_functions())
    header = open(os.path.join(ROOT, "include", "niti_hip.h")).read()
    types = set(re.findall(r"}\s*(niti_[a-z0-9_]+)\s*;", header))  # typedef struct {...} niti_x;
    used = set(re.findall(r"\b(niti_[a-z0-9_]+)\s*\(", adapter_source())) - types
    assert used and used <= declared, used - declared
