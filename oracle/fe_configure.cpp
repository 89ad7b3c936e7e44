// Stands in for AS_configure (AS_global.C needs the build-generated canu_version.H): the
// reference findErrors' main() calls it first and goes on with the argument count it returns.
int AS_configure(int argc, char **argv) { (void)argv; return argc; }
