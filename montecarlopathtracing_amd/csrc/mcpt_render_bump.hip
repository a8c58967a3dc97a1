// mcpt_render_bump.hip — k_render's mapped forms (normal maps, on the textured
// forms), a translation unit of their own: mcpt_device.hip compiled with
// MCPT_BUMP_TU keeps the kernel templates and the one table the main unit
// reaches them through (bump_render_fn) and drops everything else, so the
// device compile's four parts run side by side.  Built with mcpt_device.hip's
// flags.
#ifndef MCPT_BUMP_TU
#define MCPT_BUMP_TU
#endif
#include "mcpt_device.hip"
