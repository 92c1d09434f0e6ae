"""Writes the corpus of tools/png_host_fuzz.cpp: the hostile inputs of tests/png_cases.py (a 17 x 9 RGB file and its 4-bit palette
twin cut at every byte and with every bit of their zlib streams flipped, the hand-made invalid streams, one file per parser refusal)
and the valid set.

    python tools/png_fuzz_corpus.py corpus.bin
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def corpus():
    import png_cases as PC

    return list(PC.hostile_corpus()) + [f for _, f in PC.valid_cases()]


def main(path):
    import png_cases as PC

    cases = corpus()
    with open(path, "wb") as f:
        f.write(PC.corpus_blob(cases))
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
