"""The limits on a plane's own extent, without a device (tests/test_far_frames.py holds the kernels to them on one): a destination plane
of 2^32 bytes or more is refused (32-bit store offsets), and so is a source plane of 2^32 bytes or more (32-bit fetch offsets in
ewa_strip_kernel, the 8-bit frame-pair tile and the direct kernel, and inside a tile of the frame-lane family).  Both are decided from
pitches and plane heights alone (plane_size_refusal, what validate_planes asks before a call queues anything); the test header's
jinc_debug_plane_extent_check asks the same question of a filter that has no device."""
import pytest

G32 = 1 << 32
DST = r"JincResize: destination plane larger than 4 GiB is not supported \(32-bit store offsets\)\."
SRC = r"JincResize: source plane larger than 4 GiB is not supported \(32-bit fetch offsets\)\."


@pytest.mark.parametrize("fmt,sb", [("Y8", 1), ("Y16", 2), ("Y32", 4), ("YH", 2), ("YBF", 2)])
def test_plane_extent_limits(pkg, fmt, sb):
    sw, sh, tw, th = 64, 48, 128, 96
    f = pkg.Filter(pkg.FORMATS[fmt], sw, sh, tw, th, device=-1)
    # the largest destination pitch that is still served, and the next one
    ok_d = ((G32 - 1) // th) // sb * sb
    bad_d = -(-(-(-G32 // th)) // sb) * sb
    assert ok_d * th < G32 <= bad_d * th
    f.plane_extent_check([sw * sb], [ok_d])
    with pytest.raises(pkg.JincError, match=DST):
        f.plane_extent_check([sw * sb], [bad_d])
    # source: pitch * (rows - 1) + one row of samples
    ok_s = ((G32 - 1 - sw * sb) // (sh - 1)) // sb * sb
    bad_s = -(-(-(-(G32 - sw * sb) // (sh - 1))) // sb) * sb
    assert ok_s * (sh - 1) + sw * sb < G32 <= bad_s * (sh - 1) + sw * sb
    f.plane_extent_check([ok_s], [tw * sb])
    with pytest.raises(pkg.JincError, match=SRC):
        f.plane_extent_check([bad_s], [tw * sb])
    f.close()


def test_plane_extent_limits_go_plane_by_plane(pkg):
    """The chroma planes of a 4:2:0 frame have their own heights: a pitch that the luma plane's 96 rows cannot take is fine for 48."""
    f = pkg.Filter(pkg.FORMATS["YUV420P8"], 64, 48, 128, 96, device=-1)
    luma_bad = -(-G32 // 96)
    with pytest.raises(pkg.JincError, match=DST):
        f.plane_extent_check([64, 32, 32], [luma_bad, 64, 64])
    f.plane_extent_check([64, 32, 32], [128, luma_bad, luma_bad])
    with pytest.raises(pkg.JincError, match=DST):
        f.plane_extent_check([64, 32, 32], [128, 64, 2 * luma_bad])
    with pytest.raises(pkg.JincError, match=SRC):
        f.plane_extent_check([64, 32, -(-G32 // 23)], [128, 64, 64])
    f.close()
