/* oracle/ref_compat/avisynth_c.h -- TEST INFRASTRUCTURE ONLY: what the reference implementation's sources need on top of
 * this project's own declaration of the AviSynth+ C API (plugin/compat/avisynth_c.h), so that oracle/build_ref.py can
 * compile them together with tests/mock_avs/mock_host.cpp into oracle/_ref/libref_mock_avs.so.
 *
 * The reference and the mock host are compiled against this one header, so struct layouts and enum values agree by
 * construction: what the resulting binary pins is the reference's arithmetic and argument handling, NOT binary
 * compatibility with a real AviSynth+ (whose SDK header this is not).
 */
#ifndef JINCRESIZE_REF_COMPAT_AVISYNTH_C_H
#define JINCRESIZE_REF_COMPAT_AVISYNTH_C_H

#include "../../plugin/compat/avisynth_c.h"

#define AVS_FORCEINLINE inline __attribute__((always_inline))

#ifdef __cplusplus
extern "C" {
#endif

/* colour-family predicates: external, answered by the mock host from its own pixel_type encoding */
int avs_is_420(const AVS_VideoInfo* vi);
int avs_is_422(const AVS_VideoInfo* vi);
int avs_is_444(const AVS_VideoInfo* vi);
int avs_is_yv411(const AVS_VideoInfo* vi);

/* the plugin's entry point: declared here so that its definition gets C linkage and is exported */
AVSC_EXPORT const char* AVSC_CC avisynth_c_plugin_init(AVS_ScriptEnvironment* env);

#ifdef __cplusplus
}
#endif
#endif
