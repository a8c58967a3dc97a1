// mcpt_render_texture.hip — k_render's textured forms (on the N forms), a
// translation unit of their own: mcpt_device.hip compiled with MCPT_TEXTURE_TU
// keeps the kernel templates and the one table the main unit reaches them
// through (texture_render_fn) and drops everything else, so the device
// compile's three parts run side by side.  Built with mcpt_device.hip's flags.
#ifndef MCPT_TEXTURE_TU
#define MCPT_TEXTURE_TU
#endif
#include "mcpt_device.hip"
