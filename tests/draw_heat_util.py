"""What the draw_heatmaps tests share on the library's side: the cp_draw_heat_style record from raw values, descriptor tables that carry
the frame -> map matrix, the call of the HOST painters (cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host) on copies of the forms'
buffers, and the list of cases the CPU and the GPU test both walk."""
import ctypes

import numpy as np

import draw_heat_ref as href
import draw_ref
import draw_util

VP, LL = ctypes.c_void_p, ctypes.c_longlong
MATRIX_IDS = {"bt601": 0, "bt709": 1}


def lib(build=True):
    L = draw_util.lib_built() if build else draw_util.lib_loaded()
    L.cp_draw_heat_scratch_bytes.restype = ctypes.c_size_t
    return L


def style_struct(channels, opacity, invert, palette3, filled=None):
    """One DRAW_HEAT_STYLE record from raw values (no range check: refusals are the library's to make)."""
    from centerpose_amd import draw
    rec = np.zeros(1, draw.DRAW_HEAT_STYLE)
    rec["channels"], rec["opacity"], rec["invert"] = (channels if filled is None else filled), opacity, int(invert)
    rec["palette"][0, :, :] = 0x5A                              # behind the channels, and byte 3: never read
    rec["palette"][0, :len(palette3), :3] = np.asarray(palette3, np.uint8).reshape(-1, 3)
    return rec


def is_yuv(form):
    return form["color"] not in ("bgr", "rgb")


def table_of(forms, addresses, matrices):
    table = draw_util.table_of(forms, addresses)
    for d, T in zip(table, matrices):
        d["mi"] = np.asarray(T, np.float64).reshape(6)
    return table


def strides_of(maps):
    """The element strides of a float32 NumPy view [N, C, h, w]."""
    return [LL(s // 4) for s in maps.strides]


def host_paint(L, forms, maps, matrices, palette, opacity, invert, matrix="bt601"):
    """The host painter over copies of the forms' buffers -> the painted buffers.  maps: a float32 view [N, C, h, w] with any positive
    strides (it goes in as it lies); matrices: one T per form; palette: (B, G, R) triples."""
    yuv = is_yuv(forms[0])
    bufs = [f["buf"].copy() for f in forms]
    table = table_of(forms, [b.ctypes.data for b in bufs], matrices)
    N, C, h, w = maps.shape
    assert maps.dtype == np.float32 and N == len(forms)
    st = style_struct(C, opacity, invert, palette)
    fn = L.cp_draw_heat_yuv_frames_host if yuv else L.cp_draw_heat_frames_host
    rc = fn(table.ctypes.data_as(VP), N, VP(maps.ctypes.data), *strides_of(maps), C, h, w, st.ctypes.data_as(VP),
            *((MATRIX_IDS[matrix],) if yuv else ()))
    assert rc == 0, L.cp_last_error()
    return bufs


def crop_form(seed, H, W):
    """A crop view of a larger packed BGR frame that starts at an odd byte offset."""
    big = W + 9
    return draw_ref._form(seed, "crop of a larger hwc bgr frame, odd byte offset", "hwc", "bgr", [((2 * big + 5) * 3, (H, W, 3), (big * 3, 3, 1))])


def forms_of(kind, seed, H, W):
    """The forms of one size: packed BGR, RGB with 4 channels, BGRA with pitched rows, chw planar (two kinds), a crop of an RGB frame and a
    crop at an odd byte offset; or NV12 / NV21 / I420 planes with and without a pitch (and surfaces for even sizes)."""
    if kind == "bgr":
        return draw_ref.bgr_forms(seed, H, W) + [crop_form(seed + 6, H, W)]
    return draw_ref.yuv_forms(seed, H, W)


def cases(kind):
    """Every (name, form, maps [1, C, h, w] view, T, palette, opacity, invert, matrix) the CPU test pins to the NumPy painter and the GPU
    test runs on the device: every form of every size under every style, on both map sizes in turn, the maps as they come, as a [0::2]
    batch view or channel-permuted, the matrix fitting the frame, the identity, or mapping the whole frame outside."""
    out = []
    for s, (H, W) in enumerate(href.SIZES):
        for f, form in enumerate(forms_of(kind, 100 * s + 7 + (50 if kind == "yuv" else 0), H, W)):
            for k, (C, opacity, invert) in enumerate(href.STYLES):
                i = 31 * s + 7 * f + k
                h, w = href.MAP_SIZES[i % 2]
                seed = 1000 * s + 10 * f + k
                pal = href.fuzz_palette(seed + 1, C)
                how = i % 3
                if how == 0:
                    maps = href.fuzz_maps(seed, 1, C, h, w)
                elif how == 1:                                  # the images of a flip-test batch: every second entry
                    maps = href.fuzz_maps(seed, 3, C, h, w)[1::2]
                else:                                           # a permuted view: the channels last in memory
                    maps = np.ascontiguousarray(href.fuzz_maps(seed, 1, C, h, w).transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)
                T = (href.fit_matrix(H, W, h, w), href.OUTSIDE, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0])[(i // 3) % 3 if i % 5 else 0]
                matrix = ("bt601", "bt709")[i % 2] if kind == "yuv" else "bt601"
                out.append(("%s %dx%d C=%d a=%d inv=%d map %dx%d view %d" % (form["name"], H, W, C, opacity, invert, h, w, how), form, maps, T, pal,
                            opacity, invert, matrix))
    return out
