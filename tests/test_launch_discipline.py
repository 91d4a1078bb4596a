"""CPU: every kernel launch of the library goes through gvk::launch (GVK_LAUNCH).

A launch is recorded into a launch plan only if it goes through gvk::launch (csrc/common.hpp).  A kernel launched any other way, or a
hipMemset* / hipMemcpy* call inside the library, would run during the recording pass and be silently absent from every replay -- the
bug that turned the zero fill and the copy into kernels (csrc/runtime.hip).  This scans the comment-stripped sources: the only
direct launch sites are the two in gvk::launch and the empty kernel of the diag library, and nothing names a hipMemset* / hipMemcpy*
function.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaviko_amd", "csrc")

LAUNCH = re.compile(r"hipLaunchKernelGGL|<<<|hipLaunchKernel\b|hipLaunchCooperativeKernel\w*|hipModuleLaunch\w*|hipExtLaunch\w*|hipExtModuleLaunch\w*")
MEMOP = re.compile(r"\bhipMem(?:set|cpy)\w*")
_TOKEN = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)


def strip_comments(src):
    """Comments replaced by blanks (newlines kept, so line numbers stay); string and character literals are left alone."""
    def blank(m):
        s = m.group(0)
        return s if s[0] in "\"'" else re.sub(r"[^\n]", " ", s)
    return _TOKEN.sub(blank, src)


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    return {os.path.basename(f): open(f).read() for f in files}


def sites(pattern, text):
    """[(line number, line)] of every match of `pattern` in the comment-stripped `text`"""
    lines = strip_comments(text).split("\n")
    return [(i + 1, line.strip()) for i, line in enumerate(lines) for _ in pattern.finditer(line)]


def test_comment_stripper():
    src = 'a<<<1,2>>>(x); // hipMemsetAsync here\n/* k<<<g,b>>>()\n hipMemcpy( */ s = "// not a comment"; hipMemcpyAsync(d);\n'
    out = strip_comments(src)
    assert out.count("\n") == src.count("\n") and len(out) == len(src)
    assert [n for n, _ in sites(LAUNCH, src)] == [1]
    assert [n for n, _ in sites(MEMOP, src)] == [3]
    assert '"// not a comment"' in out and "hipMemsetAsync" not in out


def test_the_scan_finds_the_known_sites():
    """an over-eager stripper (or a moved directory) must not make the discipline test pass vacuously"""
    src = sources()
    assert len(src) > 30 and "common.hpp" in src and "runtime.hip" in src
    assert len(sites(LAUNCH, src["common.hpp"])) == 2
    assert len(sites(LAUNCH, src["runtime.hip"])) == 1
    assert MEMOP.search(src["runtime.hip"]), "runtime.hip's comment on the capture bug names hipMemsetAsync: the raw text must show it"
    assert sum("GVK_LAUNCH(" in strip_comments(t) for t in src.values()) > 20


def test_every_launch_goes_through_gvk_launch():
    found = {(name, n, line) for name, text in sources().items() for n, line in sites(LAUNCH, text)}
    by_file = {}
    for name, n, line in found:
        by_file.setdefault(name, []).append((n, line))
    assert set(by_file) == {"common.hpp", "runtime.hip"}, f"direct kernel launches outside gvk::launch: {sorted(found)}"
    # common.hpp: both inside the body of gvk::launch (the recorded closure and the launch itself)
    text = strip_comments(sources()["common.hpp"]).split("\n")
    start = next(i for i, l in enumerate(text) if re.search(r"\binline void launch\(", l)) + 1
    end = next(i for i, l in enumerate(text) if "#define GVK_LAUNCH" in l) + 1
    assert sorted(n for n, _ in by_file["common.hpp"]) == [n for n in range(start, end) if LAUNCH.search(text[n - 1])]
    assert len(by_file["common.hpp"]) == 2 and all("hipLaunchKernelGGL(kernel, grid, block, lds, stream" in l for _, l in by_file["common.hpp"])
    # runtime.hip: the empty kernel the diag library puts in place of a stream's launches
    assert len(by_file["runtime.hip"]) == 1 and "nop_kernel" in by_file["runtime.hip"][0][1], by_file["runtime.hip"]


def test_no_memset_or_memcpy_call_in_the_library():
    found = [(name, n, line) for name, text in sources().items() for n, line in sites(MEMOP, text)]
    assert not found, f"hipMemset* / hipMemcpy* inside the library is not recorded into launch plans (use gvk_memset_async / gvk_copy_async): {found}"
