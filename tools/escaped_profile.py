"""What AVR_ESCAPED=1 does to the archives' sizes, on the CPU build of the command line (tests/cpu_recode.py: the stand-in for the batch
calls, no GPU needed): the two golden clips and every case of the generated corpus (tests/h264_corpus.py), compressed without and with
the switch.  Every archive with the switch is decompressed again and compared with its file.  There is no threshold: the figures are
what DESIGN.md quotes.  Prints one JSON line and writes it to --out.

  python tools/escaped_profile.py [--out profiles/escaped_recode.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import avrecode_ms_amd as avr
    import cpu_recode
    import damaged_recode as dmg
    import h264_corpus as corpus
    import oracle_lib
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    host.t_init_states.restype = None
    oracle = oracle_lib.load_oracle()
    exe = cpu_recode.build_cached()
    result = {"tool": "escaped_profile", "files": {}}
    with tempfile.TemporaryDirectory() as d:
        files = {name + ".mp4": cpu_recode.golden(name) for name in ("realshort", "cockatoo")}
        files.update({name + ".264": corpus.build(name, oracle, host)[0] for name in corpus.CASE_NAMES})
        for name, data in files.items():
            src = os.path.join(d, name)
            with open(src, "wb") as f:
                f.write(data)
            r = {"bytes": len(data)}
            for tag, value in (("off", "0"), ("on", "1")):
                dst = os.path.join(d, name + "." + tag)
                env = dict(os.environ, AVR_ESCAPED=value, AVR_MODEL_HOOKS="0")
                for k in ("AVR_DIGEST", "AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS"):
                    env.pop(k, None)
                subprocess.run([exe, "compress", src, dst], check=True, capture_output=True, env=env)
                with open(dst, "rb") as f:
                    archive = f.read()
                blocks = dmg.parse(archive)
                r[tag] = {"archive_bytes": len(archive), "coded_blocks": sum(dmg.has(b, 4) for b in blocks), "escaped_blocks": sum(dmg.has(b, 7) for b in blocks),
                          "literal_bytes": sum(len(dmg.get(b, 2)) for b in blocks if dmg.has(b, 2))}
                if tag == "on":
                    subprocess.run([exe, "decompress", dst, dst + ".back"], check=True, capture_output=True, env=env)
                    with open(dst + ".back", "rb") as f:
                        assert f.read() == data, name
            result["files"][name] = r
    corpus_files = [r for n, r in result["files"].items() if n.endswith(".264")]
    result["corpus"] = {tag: {k: sum(r[tag][k] for r in corpus_files) for k in ("archive_bytes", "coded_blocks", "escaped_blocks", "literal_bytes")} for tag in ("off", "on")}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
