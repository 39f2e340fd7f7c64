"""CPU: the device symbol a launcher notes for the profiler (esr_note_kernel) must be the one rocprofv3 prints -- EVERY template argument,
defaulted ones included -- because tools/pmc_traffic.py and bench.py's roofline leg join the two by name.  Round 6: conv64m_kernel gained two
template parameters, RFDN's launchers kept noting three, the join dropped the model's three dominant launches and the bench line's `traffic`
went null.  This test counts: template parameters of each __global__ kernel in csrc/ against the arguments of every name noted for it."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ntire2022_esr_amd", "csrc")


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<([":
            depth += 1
        elif ch in ">)]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _sources(strip=False):
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".inc", ".h")):
            text = open(os.path.join(CSRC, f)).read()
            if strip:      # comments and preprocessor lines may stand between `template <...>` and `__global__`
                text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
                text = re.sub(r"//[^\n]*", " ", text)
                text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
            yield f, text


def test_noted_kernel_names_carry_every_template_argument():
    kernels = {}       # name -> number of template parameters (0: not a template)
    tmpl = re.compile(r"(?:template\s*<((?:[^<>]|<[^<>]*>)*)>\s*)?__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?void\s+(\w+)\s*\(")
    for _, text in _sources(strip=True):
        for m in tmpl.finditer(text):
            kernels[m.group(2)] = len(_split_top(m.group(1))) if m.group(1) else 0
    assert len(kernels) >= 20, sorted(kernels)
    noted = []
    for f, text in _sources():
        for m in re.finditer(r'esr_note_kernel\("([^"]*)"', text):
            noted.append((f, m.group(1)))
    assert len(noted) >= 25, noted
    seen = set()
    for f, fmt in noted:
        for part in fmt.split(" + "):
            m = re.fullmatch(r"(\w+)(?:<(.*)>)?", part)
            assert m, (f, fmt)
            name, args = m.group(1), m.group(2)
            assert name in kernels, (f, fmt, "no such __global__ kernel in csrc/")
            n = len(_split_top(args)) if args is not None else 0
            assert n == kernels[name], (f, fmt, f"{name} has {kernels[name]} template parameters, the noted name carries {n}")
            seen.add(name)
    # every kernel of the product path that is launched through esr_run_ops is noted somewhere (research / probe kernels are not)
    for must in ("conv64m_kernel", "rfdb_tail_kernel", "rlfb_chain_kernel", "wino8_f32_kernel", "wino_f32_kernel", "imdb_tail_kernel",
                 "conv_s16_kernel", "conv_f32_kernel", "esa_apply_mfma_kernel", "pack_input_kernel"):
        assert must in seen, must


def _body(text, signature):
    """the brace-balanced body that follows `signature` in `text`, as a (start, end) span"""
    at = text.index(signature)
    start = text.index("{", at)
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return start, i + 1
    raise AssertionError(signature)


def test_launch_boilerplate_has_one_definition():
    """The host code around a launch was copied from launcher to launcher and the copies drifted (a per-process flag where the LDS opt-in
    is per device, a swallowed error, a NaN rounded differently by one packer).  Each piece now has ONE definition -- esr_lds_optin and
    esr_check_launch (esr_hip.hip), esr_lds_optin_flags and esr_host_to16 (esr_internal.h) -- and this test keeps a new launcher from
    bringing a copy back.  Text with comments stripped; string literals are blanked as well where a CALL is counted (the opt-in's error
    message names the call it reports)."""
    src = dict(_sources(strip=True))
    code = {f: re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', t) for f, t in src.items()}

    def sites(texts, needle):
        return [(f, m.start()) for f, t in texts.items() for m in re.finditer(needle, t)]

    # one opt-in to more than 64 KB of dynamic LDS: the call inside esr_lds_optin
    lo, hi = _body(code["esr_hip.hip"], "int esr_lds_optin(esr_lds_optin_flags& flags")
    calls = sites(code, r"hipFuncSetAttribute\s*\(")
    assert len(calls) == 1 and calls[0][0] == "esr_hip.hip" and lo < calls[0][1] < hi, calls
    lo, hi = _body(src["esr_hip.hip"], "int esr_lds_optin(esr_lds_optin_flags& flags")
    assert all(f == "esr_hip.hip" and lo < at < hi for f, at in sites(src, r"hipFuncSetAttribute\s*\(")), "named outside esr_lds_optin"
    # one launch check
    lo, hi = _body(src["esr_hip.hip"], "int esr_check_launch(const char* what)")
    got = sites(src, r"hipGetLastError")
    assert got and all(f == "esr_hip.hip" and lo < at < hi for f, at in got), got
    # one host rounding to bf16 (the constant of its round-to-nearest-even add)
    got = sites(src, r"0x7fffu\b")
    assert len(got) == 1 and got[0][0] == "esr_internal.h", got
    # one per-device flag array: the helper's type
    lo, hi = _body(src["esr_internal.h"], "struct esr_lds_optin_flags")
    got = sites(src, r"std::atomic<\s*unsigned\s*>\s*\w*\s*\[")
    assert len(got) == 1 and got[0][0] == "esr_internal.h" and lo < got[0][1] < hi, got
