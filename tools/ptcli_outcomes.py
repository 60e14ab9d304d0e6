#!/usr/bin/env python3
"""The outcomes of ptcli's command line, without a GPU: what the option loop, the combination rules and the exits between loading the scene and rendering
answer, over a generated matrix of command lines.

    tools/ptcli_outcomes.py record  PTCLI tests/golden/ptcli_outcomes.tsv    # re-record after a flag was added or changed on purpose
    tools/ptcli_outcomes.py compare PTCLI OTHER_PTCLI                        # status, stdout and stderr of two builds over the whole matrix

The matrix: with --config at a file that does not exist (nothing is read, no device is touched) every flag alone, every flag without its value, every
value-taking flag with each of BAD_VALUES, every unordered pair of flags, and every pair beside --denoise; then dry runs (-n, --root at the package) of the
package's data/config_*.toml with the flags whose checks need the loaded scene, and --denoise without -n on the configs the adaptive path refuses.
--spectral-bins is never paired with --devices 0: that one answer depends on the machine's device count.

The recording holds one row per distinct (status, first line of stderr): the shortest command line that reaches it, the status, the line; tab separated,
{pkg} for the package directory and {out} for an output directory.  tests/test_ptcli_outcomes.py replays it."""
import glob
import itertools
import os
import re
import shlex
import subprocess
import sys
import tempfile

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-pathtracer_amd")
NO_CONFIG = ["--config", "/nonexistent/config.toml"]
BARE = ["-n", "--dry-run", "--write-film", "--denoise", "--demodulate-albedo", "--demodulate-bins", "--denoise-resident", "--denoise-assemble", "--path-passes",
        "--denoise-path-passes"]
MASKS = ["1", "0x3"]
VALUED = {   # flag: its valid values
    "--config": ["/nonexistent/other.toml"], "--scene": ["scene.toml"], "--stdout-log-level": ["info"], "--write-log-level": ["info"], "--root": ["/nonexistent"],
    "--output-dir": ["/nonexistent/out"], "--seed": ["7"], "--hero-wavelengths": ["4"], "--adaptive": ["0.1"], "--devices": MASKS, "--guide-samples": ["2"],
    "--guide-chain": ["3"], "--guide-alpha-max": ["0.05"], "--spectral-bins": ["8"], "--denoise-spectral-bins": ["8"], "--develop": ["cie", "cx,cy,cz"],
    "--develop-filter": ["f"], "--develop-subsamples": ["2"], "--spectral-devices": MASKS, "--light-group-devices": MASKS, "--light-groups": ["instance"],
    "--relamp-groups": ["material"], "--relamp-bins": ["8"], "--relamp": ["0:c"], "--relamp-gains": ["1,2"], "--denoise-light-groups": ["instance"],
    "--light-gains": ["1,2"], "--mattes": ["material"], "--matte-ranks": ["4"], "--matte-samples": ["16"],
}
BAD_VALUES = ["", "x", "0", "65", "-1", "1e40", "nan", "1,,2", "1,2,3,4,5,6,7,8,9", ":c", "8:c", "0:c,0:d", "a,b"]


def forms(flag):
    """A flag's valid spellings, each a list of arguments."""
    return [[flag, value] for value in VALUED[flag]] if flag in VALUED else [[flag]]


def parse_matrix():
    flags = BARE + list(VALUED)
    lines = [["-h"], ["--help"], NO_CONFIG, NO_CONFIG + ["--no-such-flag"]]
    for flag in flags:
        lines += [NO_CONFIG + form for form in forms(flag)]
    for flag in VALUED:
        lines.append(NO_CONFIG + [flag])
        lines += [NO_CONFIG + [flag, bad] for bad in BAD_VALUES]
    for a, b in itertools.combinations(flags, 2):
        for fa, fb in itertools.product(forms(a), forms(b)):
            lines.append(NO_CONFIG + fa + fb)
            if "--denoise" not in (a, b):
                lines.append(NO_CONFIG + fa + fb + ["--denoise"])
    return lines


def run(exe, args, out):
    """(status, stdout, stderr) with {pkg} and {out} filled in on the way in and put back on the way out."""
    pkg = os.path.realpath(PKG)
    real = [a.replace("{pkg}", pkg).replace("{out}", out) for a in args]
    p = subprocess.run([exe] + real, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=out)
    back = lambda text: text.replace(pkg, "{pkg}").replace(out, "{out}")
    return p.returncode, back(p.stdout), back(p.stderr)


def scene_matrix(exe, out):
    """The exits between loading the scene and rendering, per config of the package."""
    lines = []
    for path in sorted(glob.glob(os.path.join(PKG, "data", "config_*.toml"))):
        config = ["--root", "{pkg}", "--config", "{pkg}/data/" + os.path.basename(path), "--output-dir", "{out}"]
        dry = config + ["-n"]
        lines.append(dry)
        for mode in ("instance", "material"):
            found = re.search(r"light groups: (\d+)", run(exe, dry + ["--light-groups", mode], out)[1])
            groups = int(found.group(1)) if found else 1
            for flag, extra in (("--light-groups", []), ("--denoise-light-groups", ["--denoise"])):
                lines.append(dry + [flag, mode] + extra)
                for count in (groups, groups + 1):
                    lines.append(dry + [flag, mode, "--light-gains", ",".join(["1.5"] * count)] + extra)
            relamp = dry + ["--relamp-groups", mode, "--relamp-bins", "8"]
            lines.append(relamp)
            for count in (groups, groups + 1):
                lines.append(relamp + ["--relamp-gains", ",".join(["0.5"] * count)])
            for g in range(8):
                lines += [relamp + ["--relamp", "%d:flat_one" % g], relamp + ["--relamp", "%d:no_such_curve" % g]]
        for bins in (["--spectral-bins", "8"], ["--denoise", "--denoise-spectral-bins", "8"]):
            lines += [dry + bins + ["--develop", "cie"], dry + bins + ["--develop", "no_such_curve,flat_one,flat_one"], dry + bins + ["--develop", "flat_one,flat_one,flat_one"],
                      dry + bins + ["--develop", "cie", "--develop-filter", "no_such_curve"], dry + bins + ["--develop", "cie", "--develop-filter", "flat_one"]]
        lines += [dry + ["--path-passes"], dry + ["--stdout-log-level", "info"], dry + ["--stdout-log-level", "error"], dry + ["--denoise"]]
        # without -n a --denoise run reaches the device unless the adaptive path refuses a setting first: only the configs it refuses are run
        samples = [int(s) for s in re.findall(r"min_samples = (\d+)", open(path).read())]
        if "Naive" in open(path).read() or any(s % 10 for s in samples):
            lines += [config + ["--denoise"], config + ["--denoise", "--adaptive", "0.1"]]
    return lines


def outcomes(exe):
    with tempfile.TemporaryDirectory() as out:
        lines = parse_matrix() + scene_matrix(exe, out)
        return lines, [run(exe, args, out) for args in lines]


def record(exe, tsv):
    lines, results = outcomes(exe)
    shortest = {}
    for args, (status, _, err) in zip(lines, results):
        key = (status, err.split("\n")[0])
        if "\t" in key[1]:
            sys.exit("a tab in %r" % (key,))
        if key not in shortest or (len(args), len(" ".join(args))) < (len(shortest[key]), len(" ".join(shortest[key]))):
            shortest[key] = args
    with open(tsv, "w") as f:
        for (status, err), args in sorted(shortest.items(), key=lambda item: (item[0][0], item[1])):
            f.write("%s\t%d\t%s\n" % (" ".join(shlex.quote(a) for a in args), status, err))
    print("%d command lines, %d distinct outcomes written to %s" % (len(lines), len(shortest), tsv))


def compare(exe, other):
    with tempfile.TemporaryDirectory() as out:
        lines = parse_matrix() + scene_matrix(exe, out)
        different = 0
        for args in lines:
            a, b = run(exe, args, out), run(other, args, out)
            if a != b:
                different += 1
                print("DIFFERENT: %s\n  %r\n  %r" % (" ".join(shlex.quote(x) for x in args), a, b))
    print("%d command lines compared, %d different" % (len(lines), different))
    return 1 if different else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "record":
        record(os.path.abspath(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])))
    else:
        sys.exit(__doc__)
