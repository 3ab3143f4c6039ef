"""Host emulation of the three LDS-tiled FFT passes of the fluid metric (no GPU needed).

lagomorph_amd/csrc/fft_lds.hpp writes every phase between two workgroup barriers as a function of
(phase, thread id); tests/native/fft_emul.hip runs those phases for all thread ids in turn and
compares with a double-precision DFT + the per-frequency operator (cuda/metric.cu:103-160)."""
import native_build


@native_build.needs_hipcc
def test_fft_passes_host_emulation(tmp_path):
    r = native_build.run(native_build.build(tmp_path, "fft_emul.hip", fp_contract_off=False, wall=False, werror=False,
                                            extra=native_build.GFX950, compiler="hipcc"))
    assert "all ok" in r.stdout
