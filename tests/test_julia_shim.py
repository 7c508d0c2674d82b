"""The Julia shim (iterativesolvers.jl_amd/julia/MIK.jl) cannot be executed here (no Julia toolchain), so it is kept in
step with the C ABI and with the tested Python mirror STATICALLY: every `ccall((:sym, libmik), ...)` must name a symbol
of include/mik.h with the right number of arguments, and the call sequences of the functions that replace reference
methods must equal the sequences api.py issues for the same methods."""
import os
import re

from conftest import ROOT

JL = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "julia", "MIK.jl")).read()
CCALL = re.compile(r"ccall\(\(:(\w+), libmik\),\s*(\w+),\s*\(")


def ccalls(text):
    """[(symbol, return type, number of argument types)] in source order"""
    out = []
    for m in CCALL.finditer(text):
        i, depth, start = m.end(), 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        types = text[start:i - 1]
        # split on top-level commas (Ref{Ptr{Cvoid}} contains none, NTuple would)
        n, d = (1 if types.strip().rstrip(",").strip() else 0), 0
        for ch in types.strip().rstrip(","):
            d += {"{": 1, "(": 1, "}": -1, ")": -1}.get(ch, 0)
            n += ch == "," and d == 0
        out.append((m.group(1), m.group(2), n))
    return out


def julia_function(name):
    """source text of `function <name>(...) ... end` (first definition)"""
    i = JL.index("function " + name)
    j = JL.index("\nend\n", i)
    return JL[i:j]


def test_every_ccall_matches_the_c_abi(pkg):
    sig = pkg._lib.SIGNATURES
    calls = ccalls(JL)
    assert len(calls) >= 40
    for sym, ret, nargs in calls:
        assert sym in sig, f"MIK.jl calls {sym}, which include/mik.h / _lib.py do not declare"
        assert nargs == len(sig[sym][1]), f"{sym}: MIK.jl passes {nargs} arguments, the C ABI takes {len(sig[sym][1])}"
        assert ret in ("Cint", "Cstring"), (sym, ret)
        assert (ret == "Cstring") == (sym == "mik_last_error")
    # the reference-facing surface is bound
    bound = {c[0] for c in calls}
    for must in ("mik_csr_create", "mik_spmv", "mik_dot", "mik_nrm2", "mik_axpy", "mik_xpby", "mik_sub", "mik_scal", "mik_divide", "mik_fill",
                 "mik_copy", "mik_cg_create", "mik_cg_create_op", "mik_cg_iterate", "mik_cg_iterate_many", "mik_cg_state", "mik_gmres_create",
                 "mik_gmres_create_op", "mik_gmres_iterate", "mik_gmres_state", "mik_gmres_create_partitioned", "mik_comm_create",
                 "mik_cgd_create", "mik_cgd_set_halo_plan", "mik_cgd_set_comm", "mik_cgd_init", "mik_cgd_iterate_many"):
        assert must in bound, must


def test_call_sequences_equal_the_python_mirror():
    """the C calls behind cg_iterator! / iterate / gmres_iterable! in MIK.jl, in order, are the ones api.py makes"""
    api = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "api.py")).read() + "\n" + open(os.path.join(ROOT, "iterativesolvers.jl_amd", "extras.py")).read()

    def py_calls(cls, method):
        i = api.index(f"class {cls}")
        j = api.index(f"    def {method}(", i)
        k = api.index("\n    def ", j + 10)
        return re.findall(r"lib\(\)\.(mik_\w+)\(", api[j:k])
    jl = lambda f: [c[0] for c in ccalls(julia_function(f)) if not c[0].endswith("_destroy")]      # finalizers aside
    assert jl("IterativeSolvers.cg_iterator!") == ["mik_cg_create", "mik_cg_create_op"] == py_calls("CGIterable", "__init__")
    assert jl("Base.iterate(it::HipCGIterable") == ["mik_cg_iterate"] == py_calls("CGIterable", "iterate")
    assert jl("refresh!(it::HipCGIterable") == ["mik_cg_state"] == py_calls("CGIterable", "_refresh")
    assert jl("IterativeSolvers.gmres_iterable!") == ["mik_gmres_create", "mik_gmres_create_op"] == py_calls("GMRESIterable", "__init__")
    assert jl("Base.iterate(g::HipGMRESIterable") == ["mik_gmres_iterate"] == py_calls("GMRESIterable", "iterate")
    assert jl("refresh!(g::HipGMRESIterable") == ["mik_gmres_state"] == py_calls("GMRESIterable", "_refresh")
    # the widened solvers: one C call per iteration on both sides (the Python mirror keeps the statement-by-statement path next to it)
    assert jl("IterativeSolvers.bicgstabl_iterator!") == ["mik_bicgstab_create"] == py_calls("BiCGStabIterable", "__init__")
    assert jl("Base.iterate(it::HipBiCGStabIterable") == ["mik_bicgstab_step"] == py_calls("BiCGStabIterable", "iterate")[:1]
    assert jl("IterativeSolvers.minres_iterable!") == ["mik_minres_create"] == py_calls("MINRESIterable", "__init__")
    assert jl("Base.iterate(m::HipMINRESIterable") == ["mik_minres_step"] == py_calls("MINRESIterable", "iterate")[:1]
    assert jl("IterativeSolvers.idrs_iterable!") == ["mik_idrs_create"] == py_calls("IDRSIterable", "__init__")
    assert jl("Base.iterate(it::HipIDRSIterable") == ["mik_idrs_step"] == py_calls("IDRSIterable", "iterate")[:1]
    # adjoint(A) for lsqr! / lsmr! / qmr!: a second upload of the same arrays with is_csc = 0 on both sides
    wa = julia_function("with_adjoint")
    assert "pointer(A.colptr), pointer(A.rowval), pointer(A.nzval), 1, 0, h)" in wa and "size(A, 2), size(A, 1), nnz(A)" in wa
    i = api.index("def with_adjoint")
    assert "is_csc=False" in api[i:api.index("return A", i)]


def test_shim_has_no_silent_scalar_fallback_and_reference_defaults():
    assert "Array(v)[i]" in JL and "scalar_indexing_allowed[] || error(" in JL          # getindex fails loudly unless allowed
    assert "LinearAlgebra.ldiv!(y::HipVector{T}, P::HipJacobi{T}, x::HipVector{T})" in JL
    assert "Base.BroadcastStyle(::Type{<:HipVector}) = HipStyle()" in JL
    part = julia_function("gmres_iterable_partitioned!")
    assert "restart::Int = min(20, n_global)" in part and "maxiter::Int = n_global" in part and "orth_meth::OrthogonalizationMethod = ModifiedGramSchmidt()" in part
    # every finalizer that hands a context to the library checks that the context is still alive
    for m in re.finditer(r"finalizer\((\w+) -> ([^\n]+)", JL):
        assert "alive(" in m.group(2), m.group(0)


# ---- struct layouts: the Julia mirrors (and the ctypes mirrors) against offsetof / sizeof from a compiled C probe --------------------------------
JL_SIZES = {"Cint": (4, 4), "Int32": (4, 4), "Int64": (8, 8), "Int": (8, 8), "Cdouble": (8, 8), "Float64": (8, 8), "UInt8": (1, 1)}
C_MIRRORS = {"MikOperator": ("mik_operator", ["dtype", "n", "csr", "mul", "user"]),
             "MikPrecond": ("mik_precond", ["diag", "ldiv", "user"]),
             "Partition": ("mik_partition", ["rank", "nranks", "n_ext", "x_ext", "send_idx", "n_send", "send_buf", "halo", "reduce", "user", "link"]),
             "DeviceInfo": ("mik_device_info", ["device", "compute_units", "xcds", "wavefront_size", "lds_bytes_per_cu", "l2_bytes", "hbm_bytes", "arch",
                                                "planned_compute_units", "planned_xcds", "xcd_maps", "resident_workgroup_cap", "gs_single_launch_max_segments",
                                                "gs_xcd_local_max_workgroups", "sweep_grid_cap", "mgs_resident_max_segments", "reserved"])}


def julia_type_layout(t):
    """(size, alignment) of an isbits Julia field type, laid out like C"""
    t = t.strip()
    if t.startswith("Ptr{"):
        return 8, 8
    m = re.fullmatch(r"NTuple\{(\d+),\s*(\w+)\}", t)
    if m:
        sz, al = JL_SIZES[m.group(2)]
        return int(m.group(1)) * sz, al
    return JL_SIZES[t]


def julia_struct(name):
    """[(field, offset, size)] + total size of `struct <name> ... end` in MIK.jl, by the C layout rules Julia applies to isbits structs"""
    m = re.search(rf"^struct {name}\b[^\n]*\n(.*?)^end", JL, flags=re.S | re.M)
    assert m, name
    off, out, maxal = 0, [], 1
    for line in m.group(1).splitlines():
        line = line.split("#")[0].strip()
        if not line:
            continue
        fname, ftype = line.split("::")
        sz, al = julia_type_layout(ftype)
        off = (off + al - 1) // al * al
        out.append((fname.strip(), off, sz))
        off += sz
        maxal = max(maxal, al)
    return out, (off + maxal - 1) // maxal * maxal


def c_probe(tmp_path):
    """{struct: ([(field, offset, size)], sizeof)} printed by a C program compiled against include/mik.h"""
    import json
    import subprocess
    body = []
    for cname, fields in C_MIRRORS.values():
        items = ", ".join(f'[\\"{f}\\", %zu, %zu]' for f in fields)
        args = ", ".join(f"offsetof({cname}, {f}), sizeof((({cname} *)0)->{f})" for f in fields)
        body.append(f'printf("\\"{cname}\\": [[{items}], %zu]", {args}, sizeof({cname}));')
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"mik.h\"\nint main(void) { printf(\"{\"); " + ' printf(", "); '.join(body) + ' printf("}\\n"); return 0; }\n'
    c = tmp_path / "probe.c"
    c.write_text(src)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    return json.loads(subprocess.check_output([str(exe)], text=True))


def test_mirrored_structs_have_the_c_layout(pkg, tmp_path):
    """VERDICT r5 #6a: field order, offsets, widths and total size of every struct MIK.jl and _lib.py mirror from include/mik.h, against offsetof /
    sizeof of a C probe compiled here (Julia lays isbits structs out like C; a swapped or narrowed field would corrupt the callback table silently)"""
    import ctypes as C
    probe = c_probe(tmp_path)
    ct = {"mik_operator": pkg._lib.MikOperator, "mik_precond": pkg._lib.MikPrecond, "mik_partition": pkg._lib.MikPartition, "mik_device_info": pkg._lib.MikDeviceInfo}
    for jname, (cname, _fields) in C_MIRRORS.items():
        cf, csize = probe[cname]
        jf, jsize = julia_struct(jname)
        assert [(o, s) for _, o, s in jf] == [(o, s) for _, o, s in cf], (jname, jf, cf)
        assert jsize == csize, (jname, jsize, csize)
        py = ct[cname]
        assert C.sizeof(py) == csize and [(getattr(py, f).offset, getattr(py, f).size) for f, _ in py._fields_] == [(o, s) for _, o, s in cf], cname
    # the struct-typed ccall arguments are passed by reference with the mirrored type (operator / preconditioner: a nullable pointer to a Ref of it)
    assert "Ref{Partition}" in JL and "Ref{DeviceInfo}" in JL and "op = Ref(operator_struct(" in JL and "refptr(op), refptr(plref)" in JL


# ---- dispatch: the shim's methods against the reference's (no ambiguity possible) ------------------------------------------------------------------
# positional signatures of the reference methods the shim specialises (v0.9.4; checked against its sources too when ITERATIVESOLVERS_JL_SRC names a
# checkout of IterativeSolvers.jl v0.9.4 -- the table itself is what the test relies on)
REFERENCE_METHODS = {
    "cg_iterator!": ("src/cg.jl", 120, ["Any", "Any", "Any", "Any=Identity()"]),
    "gmres_iterable!": ("src/gmres.jl", 108, ["Any", "Any", "Any"]),
    "bicgstabl_iterator!": ("src/bicgstabl.jl", 27, ["Any", "Any", "Any", "Int=2"]),
    "minres_iterable!": ("src/minres.jl", 39, ["Any", "Any", "Any"]),
    "idrs_iterable!": ("src/idrs.jl", 112, ["Any", "Any", "Any", "Any", "Number", "Any", "Real", "Real", "Number"]),
}
ABSTRACT = {"Number": {"Real", "Int", "Integer"}, "Real": {"Int", "Integer"}, "Integer": {"Int"}}


def base_type(t):
    t = t.split("=")[0].strip()
    return re.sub(r"\{.*\}", "", t) or "Any"


def subtype(a, b):
    """a <: b for the handful of types that occur in these signatures (parameters ignored: HipVector{T} ~ HipVector)"""
    a, b = base_type(a), base_type(b)
    return b == "Any" or a == b or a in ABSTRACT.get(b, ())


def positional(sig):
    """['x::HipVector{T}', 'A', 'b::HipVector{T}', 'Pl = Identity()'] -> (types, number of trailing defaults)"""
    types, ndef = [], 0
    for a in sig:
        a = a.strip()
        has_default = "=" in a.split("::")[-1] if "::" in a else "=" in a
        ndef += has_default
        types.append(a.split("::")[1].split("=")[0].strip() if "::" in a else "Any")
    return types, ndef


def shim_signature(fn):
    """positional argument list of `function IterativeSolvers.<fn>(...; ...)` in MIK.jl"""
    i = JL.index(f"function IterativeSolvers.{fn}(") + len(f"function IterativeSolvers.{fn}(")
    depth, j = 1, i
    while depth:
        depth += {"(": 1, ")": -1}.get(JL[j], 0)
        j += 1
    inside = JL[i:j - 1].split(";")[0]
    args, d, cur = [], 0, ""
    for ch in inside:
        d += {"{": 1, "(": 1, "}": -1, ")": -1}.get(ch, 0)
        if ch == "," and d == 0:
            args.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        args.append(cur)
    return [a.strip() for a in args]


def test_specialised_methods_are_strictly_more_specific_than_the_reference():
    """VERDICT r5 #6b: for every arity a method with defaults generates, the shim's positional types are subtypes of the reference's with at least
    one strict -- Julia then picks the shim's method for device vectors and can never report an ambiguity against the reference's"""
    for fn, (path, line, ref_sig) in REFERENCE_METHODS.items():
        ref_types, ref_def = positional([f"a{i}::{t}" if not t.startswith("Any") else ("a%d" % i + (" = " + t.split("=")[1] if "=" in t else "")) for i, t in enumerate(ref_sig)])
        mine, my_def = positional(shim_signature(fn))
        assert len(mine) == len(ref_types) and my_def == ref_def, (fn, mine, ref_types)        # same arities generated by the defaults
        for arity in range(len(mine) - my_def, len(mine) + 1):
            a, b = mine[:arity], ref_types[:arity]
            assert all(subtype(x, y) for x, y in zip(a, b)), (fn, arity, a, b)
            assert any(base_type(x) != base_type(y) for x, y in zip(a, b)), (fn, arity, "not strictly more specific")
        assert base_type(mine[0 if fn != "idrs_iterable!" else 1]) == "HipVector"              # dispatch hangs on the solution vector, as SURVEY 8b says
        ref_file = os.path.join(os.environ.get("ITERATIVESOLVERS_JL_SRC", ""), path)
        if os.environ.get("ITERATIVESOLVERS_JL_SRC") and os.path.exists(ref_file):           # the table above still describes the reference
            text = open(ref_file).read().splitlines()[line - 1]
            assert text.startswith(f"function {fn}("), (fn, text)
            head = "\n".join(open(ref_file).read().splitlines()[line - 1:line + 2]).split("(", 1)[1].split(";")[0]
            got = [p.strip() for p in head.split(",") if p.strip()]
            assert len(got) == len(ref_sig), (fn, got)
            for g, want in zip(got, ref_sig):
                t = g.split("::")[1].split("=")[0].strip() if "::" in g else "Any"
                t = "Any" if t in ("T", "precT") else t                                       # unconstrained type parameters of src/idrs.jl:112-114
                assert t == base_type(want), (fn, g, want)
    # the one method the shim adds on a reference function with typed arguments: no overlap with the reference's containers at all
    assert "V::Vector{HipVector{T}}, w::HipVector{T}, h::AbstractVector{T}" in JL          # vs V::StridedVector{Vector{T}} (src/orthogonalize.jl:53): disjoint element types


def test_readme_says_the_julia_shim_was_never_executed():
    head = open(os.path.join(ROOT, "README.md")).read().split("\n## ")[0]
    assert "never been executed" in head and "MIK.jl" in head


def _julia_code_only(s):
    """MIK.jl without comments, strings and character literals (placeholders keep the token boundaries)"""
    out, i, n = [], 0, len(s)
    while i < n:
        if s.startswith("#=", i):
            i = s.index("=#", i) + 2
        elif s.startswith('"""', i):
            i = s.index('"""', i + 3) + 3
            out.append('""')
        elif s[i] == '"':
            j = i + 1
            while s[j] != '"':
                j += 2 if s[j] == "\\" else 1
            out.append('""')
            i = j + 1
        elif s[i] == "#":
            j = s.find("\n", i)
            i = n if j < 0 else j
        elif s[i] == "'" and i + 2 < n and (s[i + 2] == "'" or (s[i + 1] == "\\" and s[i + 3] == "'")):
            out.append("' '")
            i += 3 if s[i + 2] == "'" else 4
        else:
            out.append(s[i])
            i += 1
    return "".join(out)


def test_shim_blocks_and_brackets_balance():
    """No Julia parser exists here: at least every block opener (function / if / for / while / let / do / struct / module / begin / try / quote / macro)
    has its `end`, and (), [], {} nest -- an edit that drops or doubles one is caught on the CPU box"""
    toks = re.findall(r"[A-Za-z_][A-Za-z_0-9!]*|[\[\]\(\)\{\}]|.", _julia_code_only(JL), flags=re.S)
    stack, openers, ends = [], 0, 0
    pairs = {")": "(", "]": "[", "}": "{"}
    for k, tok in enumerate(toks):
        prev = toks[k - 1] if k else ""
        if tok in "([{":
            stack.append(tok)
        elif tok in pairs:
            assert stack and stack.pop() == pairs[tok], f"unbalanced {tok!r} near token {k}"
        elif tok in ("function", "if", "for", "while", "let", "do", "struct", "module", "begin", "try", "quote", "macro"):
            if prev in (".", ":") or (any(b in "([" for b in stack) and tok in ("for", "if")):       # field / symbol; comprehension or generator
                continue
            openers += 1
        elif tok == "end" and prev not in (".", ":") and not any(b in "([" for b in stack):          # (a[end] is an index, not a block end)
            ends += 1
    assert not stack and openers == ends and openers >= 80, (openers, ends, stack[:3])
