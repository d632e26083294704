"""basis_universal_amd -- MI355X-native hot path of the Basis Universal encoder.

Layers:
  csrc/   hand-written gfx950 HIP kernels + the C ABI (include/basisu_hip.h) -> lib/libbasisu_hip.so
  _cabi   the ctypes signatures of all three libraries, derived from the headers under include/
  capi    ctypes binding of that C ABI (no torch types cross the boundary)
  etc1s   host-side mirror of the reference's basisu_frontend over the device-resident layer
  transcode  UASTC LDR 4x4 blocks / files -> RGBA32, BC1-BC5, BC7, ASTC 4x4 on the device; ETC1S files -> RGBA32, ETC1, BC1, 16-bit pixels (host decode + device)
  stats   the reference's per-slice quality stats (Max / Mean / RMS / PSNR per channel set) of a file against its source: histograms on the device, doubles on the host; on request PSNR-HVS / PSNR-HVS-M and the SSIM figures of `basisu -compare_ssim`, bit for bit
  dds     source images straight to a DX10 .dds texture (`basisu -dds`): BC1-BC5 and seven raw pixel formats packed on the device, with mips, arrays and cubemaps; a reader of those files; .dds files with their own mip chains as sources of compress() (`compress_dds`)
  source  the compressor's source-image options on the resident raster (renormalise, swizzle, alpha policy, flip, resample; the `-normal_map` preset), in front of compress()

There is deliberately no CPU fallback anywhere in this package: if the HIP library is missing or no GPU is visible the
entry points raise.
"""
from .capi import HipLibrary, HipError, load_library, LIB_PATH  # noqa: F401
from .transcode import read_uastc_file, transcode_file, transcode_uastc_blocks, read_etc1s_file, decode_etc1s_file, transcode_etc1s_file, transcode_etc1s_image  # noqa: F401
from .stats import image_metrics, file_stats  # noqa: F401
from .dds import export_dds, pack_dds_blocks, read_dds, read_dds_source, compress_dds  # noqa: F401

__all__ = ["HipLibrary", "HipError", "load_library", "LIB_PATH", "read_uastc_file", "transcode_file", "transcode_uastc_blocks",
           "read_etc1s_file", "decode_etc1s_file", "transcode_etc1s_file", "transcode_etc1s_image", "image_metrics", "file_stats", "export_dds", "pack_dds_blocks", "read_dds",
           "read_dds_source", "compress_dds"]
