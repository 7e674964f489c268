/* stand-in for samtools' sam_opts.h: SimplePileupViewer.h only needs the type to exist */
#pragma once
typedef struct { int unused; } sam_global_args;
