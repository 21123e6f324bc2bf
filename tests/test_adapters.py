"""The drop-in adapter files (adapters/: seams B1 / B2 of SURVEY.md 8b) cannot be compiled here -- they include the
reference's headers, which need Eigen / Boost / fmt -- so they are checked as text: every ddp_hip_* call they make must
exist in include/ddp_hip/ddp_hip.h with the same number of arguments, every DDP_HIP_* constant they use must be defined
there, and the include guards must be the reference's (that is what makes the include-path seam work).  The dependency-free
URDF reader is compiled and run."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTERS = ["adapters/ddp_hip_bridge.hpp", "adapters/ddp/ddp_bwd.ipp", "adapters/ddp/ddp_fwd.ipp", "adapters/pinocchio_double.cpp"]


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _declared():
    header = _strip_comments(open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read())
    decl = {}
    for m in re.finditer(r"\b(ddp_hip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S):
        args = m.group(2).strip()
        decl[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    consts = set(re.findall(r"\b(DDP_HIP_[A-Z0-9_]+)\b", header))
    return decl, consts


def _calls(text):
    """(name, argument count) of every ddp_hip_*(...) call, matching parentheses"""
    out = []
    for m in re.finditer(r"\b(ddp_hip_[a-z0-9_]+)\s*\(", text):
        i, depth, nargs, seen = m.end(), 1, 0, False
        while depth and i < len(text):
            ch = text[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                nargs += 1
            elif not ch.isspace():
                seen = True
            i += 1
        out.append((m.group(1), nargs + 1 if seen else 0))
    return out


def test_adapter_files_exist_and_call_the_declared_abi():
    decl, consts = _declared()
    assert len(decl) > 30
    types = {"ddp_hip_ctx", "ddp_hip_model", "ddp_hip_model_storage", "ddp_hip_problem", "ddp_hip_model_handle", "ddp_hip_urdf",
             "ddp_hip_bridge"}
    n_calls = 0
    for rel in ADAPTERS:
        text = _strip_comments(open(os.path.join(ROOT, rel)).read())
        for name, nargs in _calls(text):
            if name in types:
                continue
            assert name in decl, f"{rel}: {name} is not declared in ddp_hip.h"
            assert nargs == decl[name], f"{rel}: {name} called with {nargs} arguments, declared with {decl[name]}"
            n_calls += 1
        for c in set(re.findall(r"\b(DDP_HIP_[A-Z0-9_]+)\b", text)):
            if c.endswith("_HPP"):
                continue
            assert c in consts, f"{rel}: {c} is not defined in ddp_hip.h"
    assert n_calls >= 12


def test_replacement_headers_keep_the_references_include_guards():
    # whichever of <adapters>/ddp/ddp_bwd.ipp and <reference>/include/ddp/ddp_bwd.ipp comes first on the include path wins
    bwd = open(os.path.join(ROOT, "adapters/ddp/ddp_bwd.ipp")).read()
    fwd = open(os.path.join(ROOT, "adapters/ddp/ddp_fwd.ipp")).read()
    assert "#ifndef DDP_IMPL_HPP_UBVAKU5V" in bwd and "#ifndef DDP_FWD_TCC_O5KLTLOB" in fwd      # ddp_bwd.ipp:1, ddp_fwd.ipp:1
    # the members they define are the ones declared at ddp.hpp:845-862, with the reference's parameter names and order
    for frag in ("control_feedback_t&&", "trajectory_t const&", "typename multiplier_sequence<M>::type const&", "derivative_storage_t const&",
                 "-> backward_pass_result_t<M>"):
        assert frag in bwd, frag
    for frag in ("trajectory_t&", "backward_pass_result_t<M> const&", "bool", "-> scalar_t"):
        assert frag in fwd, frag
    tu = open(os.path.join(ROOT, "adapters/pinocchio_double.cpp")).read()
    assert "template struct model_t<double>;" in tu


def test_urdf_reader_builds_and_reads_a_small_arm(tmp_path):
    exe = tmp_path / "test_urdf"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "host", "test_urdf.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode()
    assert "test_urdf: ok" in out


# ---- access specifiers of the reference members the adapters name -------------------------------------------------------
import json
import sys

GOLDEN_ACCESS = os.path.join(ROOT, "tests", "golden", "reference_member_access.json")


def _access_table():
    return json.load(open(GOLDEN_ACCESS))


def _rma():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reference_member_access as rma
    return rma


# headers of the shapes the tool meets in the reference (written for this test, not taken from it)
_HEADERS = """\
namespace ddp {
/* struct hidden_t { private: int m_a; }; */
struct plain_t {
  int m_a;                          // public: a struct's default
  struct inner_t {
   private:
    int m_b;                        // nested body: not plain_t's
  };
  char const* s = "private:";
 private:
  double m_b = 0;
  void helper(int m_c) {}
 public:
  auto dynamics_aba() const -> int { return m_b; }
 protected:
  int m_c[3];
};
class model_t {
  int m_model;                      // private: a class's default
 public:
  model_t();
  int dt;
};
}
"""


def test_reference_member_access_tool_reads_access_specifiers():
    """tools/reference_member_access.py, which makes tests/golden/reference_member_access.json from the reference's headers:
    a struct's members default to public and a class's to private, `public:` / `private:` / `protected:` switch at the
    body's own nesting depth only, and nested bodies, parameters, comments and strings hold no declarations of the struct"""
    rma = _rma()
    text = rma.strip(_HEADERS)
    assert rma.access_of(text, "plain_t", "m_a") == ("public", 4)
    assert rma.access_of(text, "plain_t", "m_b") == ("private", 11)
    assert rma.access_of(text, "plain_t", "dynamics_aba") == ("public", 14)
    assert rma.access_of(text, "plain_t", "m_c") == ("protected", 16)
    assert rma.access_of(text, "inner_t", "m_b") == ("private", 7)
    assert rma.access_of(text, "model_t", "m_model") == ("private", 19)
    assert rma.access_of(text, "model_t", "dt") == ("public", 22)
    assert rma.access_of(text, "hidden_t", "m_a") == (None, None)
    assert rma.access_of(text, "plain_t", "m_missing") == (None, None)


def test_reference_member_access_table_covers_every_used_member():
    """the committed table holds one row per reference member the tool's USED list names (the check below reads nothing
    else), in that order, each with an access specifier and a line.  After a change of the reference, regenerate it with
    `tools/reference_member_access.py <reference checkout>`"""
    rma = _rma()
    table = _access_table()
    assert [(r["header"], r["struct"], r["member"]) for r in table] == [("include/ddp/" + h, s, m) for h, s, m in rma.USED]
    for r in table:
        assert r["access"] in ("public", "private", "protected") and isinstance(r["line"], int) and r["line"] > 0, r


def test_adapters_only_name_public_members_of_the_reference():
    """Round 2's bridge read pendulum_model_t::m_mass / m_length, which are private (pendulum_model.hpp:20-26): a compile
    error nobody could see here.  Every `.m_xxx` / `->m_xxx` the free functions of the bridge and the two .ipp files name
    must be a member the table knows as public; the B2 translation unit defines model_t<double>'s own members and may
    name that class's private members, nothing else's."""
    table = _access_table()
    assert all(r["access"] in ("public", "private", "protected") for r in table), [r for r in table if r["access"] is None]
    public = {r["member"] for r in table if r["access"] == "public"}
    private = {r["member"] for r in table if r["access"] != "public"}
    assert {"m_mass", "m_length"} <= private            # the table sees what round 2 missed
    for rel in ("adapters/ddp_hip_bridge.hpp", "adapters/ddp/ddp_bwd.ipp", "adapters/ddp/ddp_fwd.ipp"):
        text = _strip_comments(open(os.path.join(ROOT, rel)).read())
        named = set(re.findall(r"(?:\.|->)\s*(m_[a-z_0-9]+)\b", text))
        for member in sorted(named):
            assert member in public or member in private, f"{rel}: {member} is not in tools/reference_member_access.py:USED"
            # a name that is private in one struct and public in another (m_model: dynamics_t vs model_t) is judged by the
            # struct it is reached through: the bridge only reaches m_model through dynamics_t::m_model (public)
            if member in private and member not in public:
                raise AssertionError(f"{rel}: names the private member {member} of the reference")
    # the other reference members the bridge reaches (non m_ names): all public
    for member in ("prob", "eq_idx", "index_begin", "index_end", "dt", "c", "second_order_finite_diff", "lfx", "lfxx",
                   "dynamics_aba"):
        assert member in public, member


def test_integration_md_listings_are_literal_excerpts():
    """INTEGRATION.md's listings had drifted from the adapter files in round 2; they are now written from the files
    (tools/sync_integration.py) and held to them here"""
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "sync_integration.py"), "--check"]).decode()
    assert "listings match" in out and int(out.split()[0]) >= 5
