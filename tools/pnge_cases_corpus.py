"""Writes the input of tools/pnge_host_check.cpp: the case list of tests/pnge_cases.py (frames at C = 1 and C = 3 with the segment size
each is to be coded at).

    python tools/pnge_cases_corpus.py cases.bin
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(path):
    import pnge_cases as EC

    with open(path, "wb") as f:
        f.write(EC.corpus_blob())
    print(f"{len(EC.cases())} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
