"""CPU check of the routing between the two kernels of k_rows_pruned.hip: frame_rows_lanes_kernel (band sums in the lanes that
computed the power terms) runs where rows_lanes_supported holds -- the default 44.1 kHz / 1024 / 64 / 32-band table -- and
frame_rows_pruned_kernel (band sums through LDS) everywhere else.  LBAudioDetectiveGetBandSumForm reads the settings, no
device; stage1_choose and its record do not know the form (the family stays "pruned").  Needs no GPU."""
import pytest

WINDOW, STRIDE = 1024, 64


def _det(lb, rate, bands=32, stride=STRIDE):
    return lb.Detective().configure(sample_rate=rate, window=WINDOW, stride=stride, bands=bands)


def test_entry_points_are_in_the_table(lb):
    from lbaudiodetective_amd import _native as N
    for name in ("LBAudioDetectiveSetBandSumForm", "LBAudioDetectiveGetBandSumForm"):
        assert name in N._SIGNATURES and hasattr(lb.lib(), name), name


def test_default_plan_takes_the_lanes_form_under_auto(lb):
    det = _det(lb, 44100)
    assert det.band_sum_form() == 2
    det.set_band_sum_form(1)
    assert det.band_sum_form() == 1
    det.set_band_sum_form(2)
    assert det.band_sum_form() == 2
    det.set_band_sum_form(0)
    assert det.band_sum_form() == 2
    with pytest.raises(lb.LBAudioDetectiveError):
        det.set_band_sum_form(3)


@pytest.mark.parametrize("rate,bands,stride", [(48000, 32, STRIDE), (96000, 32, STRIDE), (44100, 16, STRIDE), (44100, 33, STRIDE),
                                               (44100, 32, 32)])
def test_other_plans_keep_the_lds_form(lb, rate, bands, stride):
    det = _det(lb, rate, bands, stride)
    assert det.band_sum_form() == 1
    with pytest.raises(lb.LBAudioDetectiveError):
        det.set_band_sum_form(2)
    assert det.band_sum_form() == 1
    det.set_band_sum_form(1)
    det.set_band_sum_form(0)


def test_form_follows_the_settings(lb):
    """Form 2 set on the default plan does not survive as a promise on another plan: the getter reports what a call would take."""
    det = _det(lb, 44100)
    det.set_band_sum_form(2)
    det.processing_sample_rate = 48000
    assert det.band_sum_form() == 1
    det.processing_sample_rate = 44100
    assert det.band_sum_form() == 2
