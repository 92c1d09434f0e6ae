"""Writes the corpus of tools/mjps_host_fuzz.cpp: the hostile inputs of tests/mjps_cases.py (every truncation and 500 seeded
substitutions of two files without DRI), its hand-made gray scans, and one intact file without DRI per accepted form.

    python tools/mjps_fuzz_corpus.py corpus.bin
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def corpus():
    import mjpd_cases as DC
    import mjps_cases as SC

    cases = [j for _, j in SC.hostile()]
    for size in ((8, 64), (37, 50)):
        cases += [j for j, _ in SC.handmade(*size).values()]
    for form in DC.FORMS:
        for q, opt in ((1, False), (75, True), (100, False)):
            cases.append(DC.pillow_jpeg(37, 50, form, q, 0, opt))
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
