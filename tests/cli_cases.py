"""The command lines of tests/test_cli_record.py: a deterministic list of rtp_main command lines, each with an optional
RTP_DEVICES, over every flag of host/cli.cpp — alone, with good and bad values, twice, in pairs, behind the prefixes that switch the
frame drivers on, and the command lines of the per-feature CLI refusal tests.

tests/golden/make_cli_record.py records what one build of rtp_main answers to every case (refused with which code and text, or handed to
which driver); the test compares cli.cpp with the record.  The order of `cases()` is part of the record: append, never reorder.

A case is (args, rtp_devices): the elements after `rtp_main --gpu`, and the value of RTP_DEVICES or None.  The file names are relative:
run the cases in a directory that make_files() filled."""
import hashlib
import struct

PFM_W, PFM_H = 8, 4


def _vol(dims, values, magic=b"VOL1\n"):
    return magic + ("%d %d %d\n" % dims).encode() + struct.pack("<%df" % len(values), *values)


def _pfm(values):
    return ("PF\n%d %d\n-1.0\n" % (PFM_W, PFM_H)).encode() + struct.pack("<%df" % len(values), *values)


def make_files(directory):
    """grid.vol (2 x 3 x 5), other.vol (1 x 1 x 1), sky.pfm and neg.pfm (loadable; neg.pfm has a negative value), and the faulty bad.vol
    (one value short), cut.pfm (truncated) and bad.hdr (half a header).  none.vol, none.pfm and none.hdr stay absent."""
    ones = [1.0] * (PFM_W * PFM_H * 3)
    files = {"grid.vol": _vol((2, 3, 5), [0.25 * (k % 5) for k in range(30)]), "other.vol": _vol((1, 1, 1), [1.0]),
             "bad.vol": _vol((2, 3, 1), [1.0] * 5), "sky.pfm": _pfm(ones), "neg.pfm": _pfm(ones[:13] + [-1.0] + ones[14:]),
             "cut.pfm": _pfm(ones)[:-7], "bad.hdr": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 4 +X\n"}
    for name, data in files.items():
        with open(directory / name, "wb") as f:
            f.write(data)
    return sorted(files)


LOADABLE_ENV = ("sky.pfm", "neg.pfm")          # --env files that load: the environment is then made on the device

# flag → (good values, bad values); None: the flag takes no value.  "Bad" is what the flag's own check refuses or, for the flags without a
# check (--adaptive, --devices, --shard), a non-number
THREE_BAD = ["x", "1,1", "1,1,1,1", "-1,1,1", "nan,1,1", "1,1,1x", ""]
FLAGS = {
    "--aov": None, "--denoise": None, "--denoise-temporal": None, "--denoise-adaptive": None, "--denoise-adaptive-temporal": None,
    "--stop-history": None, "--lit": None, "--glossy": None, "--light-tree": None, "--fog-denoise": None,
    "--nee": (["mis", "light"], ["both", ""]),
    "--stop-rule": (["own", "near"], ["far", "Near", ""]),
    "--fog": (["0.5", "0.5:0.8", "0.5:0.8:0.3", "0"], ["x", "-1", "nan", "inf", "0.5:2", "0.5:0.5:0.99", "0.5:0.5:0.5:0.5", "0.5x", "0.5:", ""]),
    "--fog-ball": (["0,0,0,1"], ["x", "0,0,0,-1", "0,0,0", "0,0,0,1,1", "0,0,0,1x", "nan,0,0,1", "0,0,0,inf"]),
    "--fog-box": (["0,0,0,1,1,1"], ["x", "0,0,0,1,1", "0,0,0,1,1,1,1", "1,1,1,0,0,0", "0,0,0,1,0,1", "0,0,0,1,1,1x", "nan,0,0,1,1,1"]),
    "--fog-grid": (["grid.vol", "other.vol"], ["none.vol", "bad.vol", ""]),
    "--fog-heat": (["grid.vol"], ["other.vol", "none.vol", "bad.vol"]),
    "--fog-glow": (["1,1,1", "1,1,1:density", "0,0,0"], THREE_BAD + ["1,1,1:heat", ":density"]),
    "--fog-glow-sample": (["mis", "light"], ["both", ""]),
    "--fog-tint": (["1,0.5,0.25"], THREE_BAD),
    "--fog-noise-target": (["0.1", "0.1:8:8:64", "0"], ["x", "-1", "nan", "inf", "0.1:1:8:64", "0.1:8:8", "0.1:8:8:64:1", "0.1x", "0.1:8:8:64x",
                                                        "0.1:8:0:64", "0.1:8:8:4", "0.1:8:8:70000", ""]),
    "--noise-target": (["0.1"], ["x", "-1", "nan", "inf", "0.1x", ""]),
    "--noise-spp": (["8:8:64"], ["x", "1:8:64", "8:8", "8:8:64:1", "8:8:64x", "8:0:64", "8:8:4", "8:8:70000", "8x8x64"]),
    "--adaptive": (["0.1"], ["x"]),
    "--adaptive-spp": (["8:8:64"], ["x", "8:8", "8x8x64"]),
    "--env": (["sky.pfm", "sky.pfm:64"], ["none.pfm", "sky.pfm:0", "sky.pfm:5000", "sky.pfm:123456", ":64", "", "bad.vol", "cut.pfm:8", "bad.hdr"]),
    "--env-mode": (["path", "mis", "light"], ["both", ""]),
    "--env-scale": (["2"], ["x", "-1", "nan", "2x", ""]),
    "--env-up": (["y", "z"], ["x", ""]),
    "--lens": (["0.1:5"], ["x", "-1:5", "0.1:0", "0.1", "0.1:5:1", "0.1:5x", "nan:5", "0.1:inf"]),
    "--motion-blur": (["0.5"], ["x", "0", "1.5", "2", "0.5x", "nan"]),
    "--devices": (["2", "0"], ["x"]),
    "--shard": (["2", "0"], ["x"]),
    "--env-foo": None, "--denoisefoo": None,          # no flags: they begin like the two families the refusals match by their beginning
}
# the flags whose values one block of checks judged together: a faulty value of each, in both orders
BLOCKS = (("--fog-glow-sample", "--fog-glow"), ("--noise-target", "--noise-spp"), ("--fog", "--fog-ball", "--fog-box"),
          ("--env", "--env-mode", "--env-scale", "--env-up"), ("--lens", "--motion-blur"), ("--nee", "--lens"), ("--adaptive-spp", "--stop-rule"))
BOX = ["--fog-box", "0,0,0,1,1,1"]
PREFIXES = (["--lit"], ["--lit", "--fog", "0.5"], ["--lit", "--fog", "0.5"] + BOX + ["--fog-grid", "grid.vol"],
            ["--lit", "--fog", "0.5"] + BOX + ["--fog-grid", "grid.vol", "--fog-glow", "1,1,1"], ["--adaptive", "0.1"],
            ["--lit", "--noise-target", "0.1"], ["--denoise-adaptive-temporal", "--adaptive", "0.1"])


def _forms(flag, bad=True):
    """The ways to write one flag: with each good value, and (bad) with each bad one."""
    if FLAGS[flag] is None:
        return [[flag]]
    good, wrong = FLAGS[flag]
    return [[flag, v] for v in good + (wrong if bad else [])]


def _from_the_feature_tests():
    """Every command line of the per-feature CLI refusal tests (tests/test_*.py: test_cli_refusals and kin), their files under the names
    of make_files()."""
    out = []
    ad, lit = ["--adaptive", "0.3"], ["--lit", "--noise-target", "0.3"]
    sh, dat = "--stop-history", "--denoise-adaptive-temporal"
    fog = ["--lit", "--fog", "0.5"]
    box = fog + BOX
    # test_adaptive, test_aov, test_denoise, test_denoise_temporal
    out += [(["--adaptive", "0.1", *e], None) for e in (["--denoise"], ["--aov"], ["--shard", "2"], ["--devices", "2"], ["--adaptive-spp", "4x4x8"])]
    for flag in ("--aov", "--denoise", "--denoise-temporal"):
        out += [([flag, "--devices", "1"], None), ([flag, "--shard", "1"], None), ([flag], "2")]
    out += [(["--denoise", "--denoise-temporal"], None)]
    # test_adaptive_prior
    out += [(a, None) for a in ([sh], ad + [sh], lit + [sh], ad + ["--denoise-adaptive", sh], ["--denoise", sh], ["--denoise-temporal", sh],
                                ad + ["--stop-rule", "near", sh], ["--lit", "--fog", "0.1", sh], [dat, sh], ad + [dat, sh, "--denoise"],
                                lit + [dat, sh, "--lens", "0.1:10"], ad + ["--denoise-adaptive", "--denoise-temporal"],
                                ["--adaptive", "0.1", "--denoise-temporal"], ["--lit", "--denoise-temporal"], ["--adaptive", "0.1", "--stop-rule", "far"], [dat])]
    out += [(ad + [dat, sh], "2")]
    # test_adaptive_rule
    out += [(a, None) for a in (["--stop-rule", "near"], ["--stop-rule", "own"], ["--lit", "--stop-rule", "near"], ["--nee", "--stop-rule", "near"],
                                ["--noise-target", "0.3", "--stop-rule", "near"], ["--denoise", "--stop-rule", "near"], ["--adaptive", "0.1", "--stop-rule", "1"],
                                ["--adaptive", "0.1", "--stop-rule"], lit + ["--stop-rule", "Near"], lit + ["--stop-rule"],
                                ["--adaptive", "0.1", "--stop-rule", "near", "--denoise"], lit + ["--stop-rule", "near", "--aov"])]
    # test_aov_volume
    out += [(a, None) for a in (["--lit", "--fog-denoise"], ["--fog-denoise"], ["--lit"] + BOX + ["--fog-denoise"])]
    out += [(fog + ["--fog-denoise"] + e, None) for e in (["--denoise"], ["--denoise-temporal"], ["--denoise-adaptive"], [dat], ["--aov"], ["--adaptive", "0.1"],
                                                           ["--devices", "2"], ["--shard", "2"], ["--fog-noise-target", "0.3", "--aov"])]
    # test_chroma
    tint = ["--fog-tint", "0.5,1,2"]
    out += [(["--lit"] + tint, None), (fog + tint + ["--fog-noise-target", "0.1"], None), (fog + tint + ["--fog-denoise"], None)]
    out += [(fog + ["--fog-tint", v], None) for v in ("0.5,1", "0.5,-1,2", "0.5,1,2,3", "0.5,nan,2")] + [(fog + ["--fog-tint"], None)]
    # test_denoise_spp
    da = "--denoise-adaptive"
    out += [(a, None) for a in ([da], ["--denoise", da], ["--nee", da], ["--lit", da], ["--lens", "0.1:10", da], ["--noise-target", "0.3", da],
                                ad + [da, "--denoise"], ad + [da, "--denoise-temporal"], ad + [da, "--aov"], lit + [da, "--denoise"], lit + [da, "--aov"],
                                lit + [da, "--denoise-temporal"], ["--adaptive", "0.1", "--denoise"], lit + ["--denoise"], ad + [da, "--devices", "2"],
                                ad + [da, "--shard", "2"])]
    # test_denoise_temporal_spp
    out += [([dat], None), (["--denoise", dat], None), (["--nee", dat], None), (["--lit", dat], None), (["--noise-target", "0.3", dat], None),
            (["--lens", "0.1:10", dat], None), (ad + [dat], "2"), (lit + [dat], "1")]
    for mode in (ad, lit):
        out += [(mode + [dat, e], None) for e in ("--denoise", "--denoise-temporal", da, "--aov")]
        out += [(mode + [dat, *e], None) for e in (["--lens", "0.1:10"], ["--motion-blur", "0.5"], ["--devices", "2"], ["--shard", "2"])]
    out += [(ad + [da, dat, e], None) for e in ("--denoise-temporal", "--aov", "--denoise")]
    out += [(lit + [da, dat, "--denoise-temporal"], None), ([da, dat], None), (ad + [dat, "--denoise", "--denoise-temporal"], None),
            (ad + [dat, "--aov", "--devices", "2"], None)]
    # test_env
    sky = ["--env", "sky.pfm"]
    out += [(sky + e, None) for e in (["--nee"], ["--lens", "0.1:10"], ["--motion-blur", "0.5"], ["--adaptive", "0.1"], ["--denoise-temporal"], ["--devices", "2"],
                                      ["--shard", "2"], ["--env-mode", "both"], ["--env-scale", "-1"], ["--env-scale", "x"], ["--env-up", "x"])]
    out += [(sky, "2"), (["--env"], None), (["--env-mode", "mis"], None)]
    out += [(["--env", v], None) for v in ("sky.pfm:0", "sky.pfm:5000", "none.hdr", "cut.pfm:8", "bad.hdr", "neg.pfm:8")]
    # test_glossy, test_light_tree
    out += [(a, None) for a in (["--glossy"], ["--glossy", "--aov"], ["--glossy", "--lens", "0.2:12"], ["--glossy"] + sky + ["--env-mode", "path"],
                                ["--light-tree"], ["--light-tree", "--aov"], ["--light-tree", "--lens", "0.2:12"])]
    # test_glow
    glow, grid = ["--fog-glow", "0.5,1,2"], ["--fog-grid", "grid.vol"]
    out += [(a, None) for a in (["--lit"] + glow, fog + glow + ["--fog-tint", "1,2,3"], fog + glow + ["--fog-noise-target", "0.1"], fog + glow + ["--fog-denoise"],
                                box + ["--fog-glow", "0.5,1,2:density"], box + glow + ["--fog-heat", "grid.vol"],
                                box + grid + ["--fog-glow", "0.5,1,2:density", "--fog-heat", "grid.vol"], box + grid + ["--fog-heat", "grid.vol"],
                                box + grid + glow + ["--fog-heat", "other.vol"], box + grid + glow + ["--fog-heat", "none.vol"], ["--lit", "--fog", "0"] + glow,
                                fog + ["--fog-glow"])]
    out += [(fog + ["--fog-glow", v], None) for v in ("0.5,1", "0.5,-1,2", "0.5,1,2,3", "0.5,nan,2", "0.5,1,2:heat")]
    # test_glow_sampled
    fogged = ["--lit", "--fog", "0.4", "--fog-box", "-3,-3,-3,3,3,3"]
    out += [(fogged + e, None) for e in (grid + ["--fog-glow-sample", "mis"], ["--fog-glow", "1,1,1", "--fog-glow-sample", "mis"],
                                         grid + ["--fog-glow", "1,1,1", "--fog-glow-sample", "both"], grid + ["--fog-glow", "1,1,1", "--fog-glow-sample"])]
    # test_lens, test_nee
    out += [(a, None) for a in (["--lens", "0.1:10", "--denoise-temporal"], ["--motion-blur", "0.5", "--adaptive", "0.1"], ["--lens", "0.1:10", "--devices", "2"],
                                ["--motion-blur", "0.5", "--shard", "2"], ["--lens", "0.1:10", "--aov", "--devices", "1"], ["--motion-blur", "0"],
                                ["--motion-blur", "1.5"], ["--motion-blur", "x"], ["--lens", "-1:10"], ["--lens", "0.1:0"], ["--lens", "0.1"], ["--lens", "nan:10"],
                                ["--nee", "--lens", "0.1:10"], ["--nee", "light", "--motion-blur", "0.5"], ["--nee", "--adaptive", "0.1"], ["--nee", "--denoise-temporal"],
                                ["--nee", "mis", "--devices", "2"], ["--nee", "--shard", "2"], ["--nee", "both"], ["--nee", "--aov", "--devices", "1"])]
    out += [(["--lens", "0.1:10"], "2"), (["--nee"], "2")]
    # test_lit, test_lit_adaptive
    out += [(a, None) for a in (["--lit", "--adaptive", "0.1"], ["--lit", "--devices", "2"], ["--lit", "--shard", "2"], ["--lit"] + sky + ["--nee", "--shard", "2"],
                                ["--lens", "0.2:12", "--lit", "--adaptive", "0.1"], ["--lit", "--nee", "both"], ["--lit", "--lens", "x"], ["--lit", "--motion-blur", "2"],
                                ["--lit"] + sky + ["--env-mode", "both"], ["--lit", "--env-mode", "mis"], ["--noise-target", "0.3"], ["--nee", "--noise-target", "0.3"],
                                lit + ["--adaptive", "0.1"], lit + ["--aov"], ["--lit", "--noise-target"], ["--lit", "--noise-spp", "4:4:32"], ["--noise-spp", "4:4:32"])]
    out += [(["--lit"], "2")]
    out += [(["--lit", "--noise-target", v], None) for v in ("x", "-0.1", "nan", "inf")]
    out += [(lit + ["--noise-spp", v], None) for v in ("4x4x32", "4:4", "1:4:32", "4:0:32", "8:4:4", "4:4:70000", "4:4:32x")]
    # test_medium, test_volume, test_volume_adaptive
    out += [(["--fog", "0.5"], None), (fog + ["--noise-target", "0.1"], None), (["--lit", "--fog"], None), (["--lit", "--fog-ball", "0,0,0,1"], None)]
    out += [(["--lit", "--fog", v], None) for v in ("-1", "0.5:2", "0.5:0.9:0.99", "0.5:0.9x", "0.5:0.9:0.1:3", "nan")]
    out += [(fog + e, None) for e in (["--fog-ball", "0,0,0"], ["--fog-ball", "0,0,0,-1"], ["--fog-box", "0,0,0,1,1"], ["--fog-box", "0,0,0,1,0,1"],
                                      ["--fog-ball", "0,0,0,1"] + BOX, grid, ["--fog-ball", "0,0,0,1"] + grid, BOX + grid + ["--noise-target", "0.1"],
                                      BOX + ["--fog-grid"], BOX + ["--fog-grid", "none.vol"], BOX + ["--fog-grid", "bad.vol"])]
    out += [(["--lit"] + grid, None)]
    target = ["--fog-noise-target", "0.3"]
    out += [(["--lit"] + target, None), (target, None), (["--fog-noise-target"] + fog, None)]
    out += [(fog + ["--fog-noise-target", v], None) for v in ("x", "-0.1", "nan", "inf", "0.3:4:4", "0.3:1:4:32", "0.3:4:0:32", "0.3:8:4:4", "0.3:4:4:70000",
                                                              "0.3:4:4:32x", "0.3x", "")]
    out += [(fog + target + e, None) for e in (["--adaptive", "0.1"], ["--denoise"], ["--denoise-temporal"], [da], [dat], ["--aov"], ["--stop-rule", "near"],
                                               [sh], ["--noise-target", "0.3"])]
    return out


# The class of cases whose answer the move of the device objects behind the last refusal changes: under --lit, an --env
# that loads and a faulty --nee, --lens or --motion-blur value.  Without a GPU the build before the move fails in rt_env_create there.
def _moved_refusals():
    out = []
    for env in (["--env", "sky.pfm"], ["--env", "sky.pfm:64", "--env-mode", "light"]):
        for flag in ("--nee", "--lens", "--motion-blur"):
            for form in [[flag, v] for v in FLAGS[flag][1]] + ([[flag]] if flag != "--nee" else []):
                out += [["--lit"] + env + form, ["--lit"] + form + env]
    out += [["--lit", "--env", "sky.pfm", "--nee", "both", "--lens", "x"], ["--lit", "--env", "sky.pfm", "--motion-blur", "x", "--nee", "both"]]
    return out


def moved_refusal(case):
    """The text the ordered list gives a case of _moved_refusals(): --nee's check stands before --lens / --motion-blur's."""
    args = case[0]
    nee_bad = any(a == "--nee" and k + 1 < len(args) and args[k + 1] in FLAGS["--nee"][1] for k, a in enumerate(args))
    return "--nee takes mis (default) or light" if nee_bad else "--lens takes R:F (R >= 0, F > 0, finite) and --motion-blur takes S (0 < S <= 1)"


def has_faulty_lit_tail(case):
    """Does the case carry a value of --nee, --lens or --motion-blur from the lists of bad values (or --lens / --motion-blur as the last
    element)?  The recorder uses it to make sure that no case outside _moved_refusals() belongs to their class."""
    args = case[0]
    for k, a in enumerate(args):
        if a in ("--nee", "--lens", "--motion-blur"):
            if k + 1 == len(args):
                if a != "--nee":
                    return True
            elif args[k + 1] in FLAGS[a][1]:
                return True
    return False


def cases():
    plain = []
    for flag in FLAGS:
        plain.append([flag])                                              # alone, and so as the last element
        for form in _forms(flag):
            if len(form) == 2:
                plain.append(form)                                        # each good and each bad value
        if FLAGS[flag] is not None:
            good, wrong = FLAGS[flag]
            for w in wrong[:3]:
                plain += [[flag, good[0], flag, w], [flag, w, flag, good[0]]]          # twice: good then bad, bad then good
            plain.append([flag, good[0], flag, good[-1]])
            plain.append([flag, good[0], flag])                           # a good one, then as the last element
    for f in FLAGS:
        for g in FLAGS:
            plain.append(_forms(f, bad=False)[0] + _forms(g, bad=False)[0])          # every ordered pair, good values
    for block in BLOCKS:
        for f in block:
            for g in block:
                if f != g:
                    for wf in FLAGS[f][1][:2]:
                        for wg in FLAGS[g][1][:2]:
                            plain.append([f, wf, g, wg])                  # two faulty values of one block, in both orders
    for prefix in PREFIXES:
        for flag in FLAGS:
            for form in _forms(flag):
                plain.append(prefix + form)
            if FLAGS[flag] is not None:
                plain.append(prefix + [flag])
    # the oddities of the order, spelled out
    plain += [["--fog", "x", "--fog-ball", "0,0,0,1"] + BOX, ["--lit", "--fog", "x"] + BOX + ["--fog-grid", "none.vol"],
              ["--lit", "--fog", "0.5"] + BOX + ["--fog-grid", "grid.vol", "--fog-glow", "1,1,1", "--fog-heat", "other.vol"],
              ["--lit", "--fog", "0.5"] + BOX + ["--fog-grid", "grid.vol", "--fog-glow", "1,1,1", "--fog-heat", "grid.vol", "--fog-glow-sample", "light"],
              ["--lit", "--fog", "0.5"] + BOX + ["--fog-grid", "other.vol", "--fog-glow", "1,1,1:density", "--fog-glow-sample", "mis"],
              ["--env", "sky.pfm", "--light-tree"], ["--env", "sky.pfm", "--adaptive-spp", "x"], ["--env", "sky.pfm", "--denoise", "--stop-rule"],
              ["--nee", "--denoise", "--denoise-temporal"], ["--env", "sky.pfm:64", "--env", "sky.pfm"], ["--env", "sky.pfm:5000", "--env", "sky.pfm"],
              ["--env", "sky.pfm", "--env-up", "z", "--env-up", "y"], ["--env", "--lit"], ["--glossy", "--env", "sky.pfm", "--env-mode", "path", "--env-mode", "mis"],
              ["--glossy", "--env", "sky.pfm", "--env-mode"], ["--adaptive", "0.1", "--devices", "0"], ["--adaptive", "0.1", "--devices"],
              ["--adaptive", "--adaptive", "0.1"], ["--adaptive", "0.1", "--adaptive-spp"], ["--adaptive", "0.1", "--shard"], ["--shard", "--devices", "2"],
              ["--devices", "2", "--devices"], ["--aov", "--devices", "0"], ["--nee", ""], ["--nee", "--lit"], ["--lit", "--nee", "light", "--nee"],
              ["--noise-spp", "x", "--noise-target", "0.1"], ["--lit", "--noise-target", "x", "--aov"], ["--lit", "--noise-target", "0.1", "--noise-spp", "x", "--aov"],
              ["--stop-rule", "far", "--stop-rule", "near", "--adaptive", "0.1"], ["--fog-denoise", "--fog", "0.5", "--aov", "--denoisefoo"],
              ["--lit", "--fog", "0.5", "--fog-noise-target", "0.1:8:8:64", "--fog-noise-target", "0.2"], ["--lit", "--env", "none.pfm", "--lens", "x"],
              ["--lit", "--env", "neg.pfm:8"], ["--lit", "--env", "sky.pfm", "--nee", "light", "--lens", "0.1:5", "--motion-blur", "0.5", "--glossy", "--light-tree"]]
    out = [(args, None) for args in plain] + [(args, "2") for args in plain]
    out += [(["--denoise-adaptive-temporal", "--adaptive", "0.1"], ""), (["--lit"], ""), (["--devices", "3"], "0"), ([], "x"), ([], "0")]
    out += _from_the_feature_tests()
    out += [(args, None) for args in _moved_refusals()]
    return out


MOVED = {tuple(a) for a in _moved_refusals()}


def is_moved(case):
    return case[1] is None and tuple(case[0]) in MOVED


def case_id(case):
    args, devices = case
    return ("" if devices is None else "RTP_DEVICES=" + devices + " ") + " ".join(a if a else '""' for a in args)


def case_line(case):
    """One case as a line for tests/cpu_native/cli_probe.cpp: RTP_DEVICES ("-" unset, else "=" and the value), then the elements, tab-separated."""
    args, devices = case
    return "\t".join(["-" if devices is None else "=" + devices] + args)


def ids_digest(all_cases):
    return hashlib.sha256("\n".join(case_id(c) for c in all_cases).encode()).hexdigest()
