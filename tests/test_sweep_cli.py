"""`python -m openglottal_amd.cli sweep`: the flags, what is refused before a device is touched, and the two tables.  No GPU."""
import numpy as np
import pytest

from openglottal_amd import cli, sweep
from openglottal_amd.evaluate import metrics_from_counts, summarize


def test_the_flags_and_what_is_refused_early(tmp_path, capsys):
    for argv in (["sweep"], ["sweep", "--kind", "hold"], ["sweep", "--kind", "both", "--frames", "f", "--gts", "g", "--unet-weights", "u",
                                                          "--yolo-weights", "y"],
                 ["sweep", "--kind", "conf", "--frames", "f.npy", "--gts", "g.npy", "--unet-weights", "u"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
    f, g = str(tmp_path / "f.npy"), str(tmp_path / "g.npy")
    np.save(f, np.zeros((3, 8, 8, 3), np.uint8))
    np.save(g, np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(SystemExit) as e:            # before any weight is read or a device is touched
        cli.main(["sweep", "--kind", "hold", "--frames", f, "--gts", g, "--unet-weights", "none.pt", "--yolo-weights", "none.npz"])
    assert "3 frames" in str(e.value.code) and "2 masks" in str(e.value.code)


def test_rows_and_tables_from_counts(capsys):
    fc = np.array([[10, 20, 30], [0, 0, 0], [5, 5, 5]], np.int32)
    cnt = np.array([[4, 8, 1], [0, 0, 0], [0, 0, 0]], np.int32)
    agg = sweep._agg_rows(fc, cnt)
    assert agg["unet-only"]["dice"] == [metrics_from_counts(10, 20, 30)[0], 1.0, 1.0] and agg["unet-only"]["n_det"] == 0
    assert agg["yolo+unet"]["dice"] == [metrics_from_counts(4, 8, 30)[0], 1.0, 0.0] and agg["yolo+unet"]["n_det"] == 1
    assert agg["yolo+unet"]["iou"] == [metrics_from_counts(4, 8, 30)[1], 1.0, 0.0] and agg["yolo+unet"]["n_total"] == 3
    sweep.print_hold_table({0: {"agg": agg, "summary": summarize(agg)}, None: {"agg": agg, "summary": summarize(agg)}})
    out = capsys.readouterr().out
    assert "inf  YOLO+UNet" in out and "0.333" in out and "1.000 *" in out
    res = {"0.001": {"unet-only": dict(dice_mean=0.5, iou_mean=0.4, dice_ge_05=50.0, det_recall=0.0, n_det=0, n_total=3),
                     "yolo+unet": dict(dice_mean=0.25, iou_mean=0.2, dice_ge_05=33.3, det_recall=1 / 3, n_det=1, n_total=3)},
           "0.25": {"unet-only": dict(dice_mean=0.5, iou_mean=0.4, dice_ge_05=50.0, det_recall=0.0, n_det=0, n_total=3)}}
    sweep.print_conf_table(res)
    out = capsys.readouterr().out
    assert "   0.00  yolo+unet                  0.333     0.250     0.200       33.3%" in out and "Evaluated on 3 frames." in out
    assert sweep.CONF_THRESHOLDS == [0.001, 0.005, 0.01, 0.02, 0.03, 0.05, 0.10, 0.15, 0.20, 0.25] and sweep.RAW_CONF == 0.001
