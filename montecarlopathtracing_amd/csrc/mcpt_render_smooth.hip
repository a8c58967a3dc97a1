// mcpt_render_smooth.hip — k_render's smooth-shading (N) forms, a translation
// unit of their own: mcpt_device.hip compiled with MCPT_SMOOTH_TU keeps the
// kernel templates and the one table the main unit reaches them through
// (smooth_render_fn) and drops everything else, so the device compile's two
// halves run side by side.  Built with mcpt_device.hip's flags.
#ifndef MCPT_SMOOTH_TU
#define MCPT_SMOOTH_TU
#endif
#include "mcpt_device.hip"
