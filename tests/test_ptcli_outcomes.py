"""ptcli's answers without a GPU, replayed from a recording: tests/golden/ptcli_outcomes.tsv holds, for every distinct (exit status, first line of stderr) that
tools/ptcli_outcomes.py's matrix of command lines reaches — every flag alone, without its value and with malformed values, every pair of flags, and the exits
between loading the scene and rendering over the package's configs — the shortest command line that reaches it.  The option loop, the combination rules and
their order, and the messages must stay what the recording says; a flag added on purpose is re-recorded with that tool."""
import os
import shlex
import subprocess
from concurrent.futures import ThreadPoolExecutor

from util import ptcli

HERE = os.path.dirname(os.path.abspath(__file__))


def recorded():
    rows = []
    for line in open(os.path.join(HERE, "golden", "ptcli_outcomes.tsv")).read().split("\n"):
        if line:
            args, status, err = line.split("\t")
            rows.append((shlex.split(args), int(status), err))
    return rows


def test_recorded_outcomes(pkg, tmp_path):
    exe, root, out = ptcli(pkg), os.path.realpath(pkg.PACKAGE_DIR), str(tmp_path)

    def outcome(row):
        p = subprocess.run([exe] + [a.replace("{pkg}", root).replace("{out}", out) for a in row[0]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, cwd=out)
        return row[0], p.returncode, p.stderr.split("\n")[0].replace(root, "{pkg}").replace(out, "{out}")

    rows = recorded()
    assert len(rows) > 100
    with ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(outcome, rows))
    wrong = [(g, want) for g, want in zip(got, rows) if g != want]
    assert not wrong, "%d of %d outcomes differ from the recording, the first: %r" % (len(wrong), len(rows), wrong[0])


def test_help(pkg):
    for flag in ("-h", "--help"):
        p = subprocess.run([ptcli(pkg), flag], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert p.returncode == 0 and p.stdout == "" and p.stderr.startswith("usage: ptcli [--config FILE]") and "[--path-passes] [--denoise-path-passes]" in p.stderr
        assert "error:" not in p.stderr
