"""src.dmtet.geometry: dmtet_geometry is this project's (diffsound_amd.dmtet); sdf, dmtet_thickness, ... fall through
to the next ``src`` tree on sys.path."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
