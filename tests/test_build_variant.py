"""scripts/build_variant.sh (tagged A/B copies of the library) compiles exactly the Makefile's sources and links all of them.

Its own source list once fell behind csrc/Makefile: it lacked train3d_sf16, so every variant missed the split-f16 training entry
points and _lib.load() refused it ("does not export").  The script is run here with a stand-in compiler that records its calls."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cds_mvsnet_amd", "csrc")


def _makefile_srcs():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^SRCS\s*=\s*(.*)$", text, re.M)
    return m.group(1).split()


def test_build_variant_compiles_every_makefile_source(tmp_path):
    log = tmp_path / "calls.log"
    fake = tmp_path / "hipcc"
    fake.write_text('#!/bin/bash\n'
                    f'echo "$*" >> {shlex.quote(str(log))}\n'
                    'while [ $# -gt 0 ]; do if [ "$1" = -o ]; then touch "$2"; fi; shift; done\n')
    fake.chmod(0o755)
    out = tmp_path / "variants"
    env = dict(os.environ, HIPCC=str(fake), OUT=str(out))
    env.pop("ONLY", None)
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), "probe", "-DCDS_SOME_GUARD"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    calls = [c.split() for c in log.read_text().splitlines()]
    compiled = [c[c.index("-c") + 1] for c in calls if "-c" in c]
    srcs = _makefile_srcs()
    assert "train3d_sf16.hip" in srcs
    assert sorted(compiled) == sorted(srcs)
    for c in calls:
        if "-c" in c:
            assert "-DCDS_SOME_GUARD" in c and "--offload-arch=gfx950" in c and "-ffp-contract=off" in c, c
            assert ("-fno-slp-vectorize" in c) == (c[c.index("-c") + 1] in ("feat_cl.hip", "conv2d_sbf.hip")), c   # as in the Makefile
    links = [c for c in calls if "-shared" in c]
    assert len(links) == 1
    linked = sorted(os.path.basename(a) for a in links[0] if a.endswith(".o"))
    assert linked == sorted(s[:-4] + ".o" for s in srcs)
    assert links[0][links[0].index("-o") + 1] == str(out / "libcdsmvs_hip.probe.so")
    assert r.stdout.strip().endswith("libcdsmvs_hip.probe.so")
