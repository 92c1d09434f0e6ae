"""Writes the corpus of tools/mjpd_host_fuzz.cpp: the hostile inputs of tests/mjpd_cases.py (every truncation, 500 seeded substitutions
per file, damaged restart markers) and one intact file per accepted form and restart interval.

    python tools/mjpd_fuzz_corpus.py corpus.bin
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def corpus():
    import mjpd_cases as DC

    cases = [j for _, j in DC.hostile()]
    for form in DC.FORMS:
        for restart in (0, 1, 3):
            for q, opt in ((1, False), (75, True), (100, False)):
                cases.append(DC.pillow_jpeg(37, 50, form, q, restart, opt))
    return cases


def main(path):
    cases = corpus()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for j in cases:
            f.write(struct.pack("<I", len(j)) + j)
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
