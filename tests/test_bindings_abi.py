"""rtp_bindings.AMD_ABI against include/rtp_amd.h: the header is the truth.  A call without an entry "works" — ctypes passes a Python
int as a 32-bit C int and cuts a device address short — so every prototype the module calls has to be in the table with the header's
argument count, a pointer type for every pointer and c_float for every float.  Looks at the header and the table only: no library."""
import ctypes as C
import os
import re

import rtp_bindings as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "rt_status": C.c_int}
INTEGERS = (C.c_int8, C.c_uint8, C.c_int16, C.c_uint16, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_ssize_t)


def prototypes():
    """{name: (return type, [parameter types])} of every rt_* prototype in the header, the types as C text without the names."""
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)          # (#define rt_config_init(cfg) … is no prototype)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n\*]*?)\(?\b(rt_\w+)\)?[ \t\n]*\(([^()]*)\)[ \t\n]*;", text):      # name or (name)
        params = [" ".join(p.split()) for p in params.split(",")]
        if params == ["void"]:
            params = []
        # a parameter's type: what stands before its name, the stars included
        out[name] = (" ".join(ret.split()), [re.sub(r"\s*\b\w+$", "", p) if re.search(r"[\w\*]\s*\b\w+$", p) else p for p in params])
    return out


PROTOTYPES = prototypes()


def test_header_is_read_whole():
    """Every symbol the header declares (RTP_AMD_SYMBOLS: what the built library is checked for) was found as a prototype, and nothing else."""
    assert set(PROTOTYPES) == set(rb.RTP_AMD_SYMBOLS)
    assert PROTOTYPES["rt_config_init"] == ("void", ["rt_config *"]) and PROTOTYPES["rt_version_string"] == ("const char *", [])
    assert PROTOTYPES["rt_device_alloc"] == ("rt_status", ["uint64_t", "void **"])


def test_every_call_of_the_module_is_in_the_table():
    with open(rb.__file__) as f:
        source = f.read()
    called = set(re.findall(r"\.(rt_\w+)\(", source))
    # DeviceScene._call("rt_x", …), _check(…, "rt_x"), … — not "rt_x": the table's own rows
    named = set(re.findall(r"\"(rt_\w+)\"(?!:)", source)) & set(PROTOTYPES)
    assert len(called) > 25 and len(called | named) > 60
    missing = sorted(n for n in called | named if n not in rb.AMD_ABI)
    assert not missing, f"rtp_bindings calls {missing} without an AMD_ABI entry"


def test_table_matches_header():
    common = sorted(set(PROTOTYPES) & set(rb.AMD_ABI))
    assert len(common) > 60
    bad = []
    for name in common:
        ret, params = PROTOTYPES[name]
        restype, argtypes = rb.AMD_ABI[name]
        want = None if ret == "void" else C.c_char_p if ret == "const char *" else SCALARS[ret]
        if restype is not want:
            bad.append(f"{name}: returns {ret}, the table says {restype}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for k, (c, t) in enumerate(zip(params, argtypes)):
            if "*" in c:
                if t in INTEGERS or t in (C.c_float, C.c_double):
                    bad.append(f"{name}: parameter {k} is {c}, the table says {t.__name__}")
            elif t is not SCALARS[c.replace("const ", "")]:
                bad.append(f"{name}: parameter {k} is {c}, the table says {getattr(t, '__name__', t)}")
    assert not bad, "\n".join(bad)
